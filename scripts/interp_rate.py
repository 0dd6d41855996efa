#!/usr/bin/env python3
"""Rates of the blend kernels (fsea_interp_frames_* and fsea_interp_image_u8, include/fsea.h) beside a plain store stream.

1. Image form: 1000 frames of 1920 x 1080 from a 256 x 256 grid in one call (2.07 GB written).
2. Sample form: 128 frames of a 262144-byte U8 block, and of a 131072-pair F64 block (2 MiB per frame).
   Beside each, in the same process, hipMemsetAsync of the same byte count on the same buffer: the plain store stream
   the kernels are measured against (scripts/ubench/stream_rw.hip has a write-only mode, but only as a program of its own
   with a fixed 2 GiB).  The two are timed alternately, HIP events on the null stream around REPS launches after a warm-up,
   ROUNDS rounds; printed: every round's time, the best, and kernel over plain stream of the bests.
3. One nrf_interpolator_get_buffer call on a 262144-byte U8 block: median wall time, and its parts measured alone -- the
   one-frame launch (events) and the download of the frame (wall) -- beside the reference's host loop as restated in
   tests/interp_ref.py (numpy, one CPU).
The registers and LDS of the kernels are read from the shipped code object.
The measurement is one part, `run`; without it on the command line it runs as a child process under its time limit.
Usage: python scripts/interp_rate.py [run] [--image-only] [--to FILE]   (--image-only: 1. alone; a counters run names the
part, `run --image-only`, so that the profiler's child is the process that measures)"""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea, nrf  # noqa: E402
import ratelib  # noqa: E402

WARMUP, REPS, ROUNDS = 2, 3, 5
# the part's time limit: three times its wall time on an MI355X (2.2 s), rounded up to 30 s, and at least 120 s -- a first
# import of torch on a fresh machine alone can take over a minute
STEP_LIMIT_S = 120


def beside(name, nbytes, kernel, plain):
    k, p = [], []
    for _ in range(2):                       # alternately
        k += ratelib.per_round(kernel, WARMUP, REPS, ROUNDS)
        p += ratelib.per_round(plain, WARMUP, REPS, ROUNDS)
    fmt = lambda ts: " ".join("%.3f" % (t * 1e3) for t in ts)
    print("%s: %.1f MB written per launch" % (name, nbytes / 1e6))
    print("  kernel       ms: %s   best %.3f ms = %.0f GB/s" % (fmt(k), min(k) * 1e3, nbytes / min(k) / 1e9))
    print("  plain stream ms: %s   best %.3f ms = %.0f GB/s" % (fmt(p), min(p) * 1e3, nbytes / min(p) / 1e9))
    print("  kernel time / plain-stream time (bests): %.3f; plain-stream spread %.1f %%" %
          (min(k) / min(p), 100 * (max(p) - min(p)) / min(p)))


def run():
    import torch
    from tests.test_shipped_artifacts import _kernels
    from tests import interp_ref as R
    if fsea.device_count() < 1:
        sys.exit("interp_rate.py needs a GPU")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    ks = _kernels(fsea.lib_path())
    for name in ("fsea_interp_image_u8", "fsea_interp_frames_u8", "fsea_interp_frames_f64"):
        k = ks[name]
        print("%s: %d VGPRs, %d SGPRs, %d bytes of static LDS, %d bytes of scratch" %
              (name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]))
    print("fsea_interp_image_u8 at 1920 x 1080 from 256 x 256: 5376 bytes of dynamic LDS (column table 3840, two slots x 3 x 256)")
    rng = np.random.default_rng(1)

    def plain(buf):
        return lambda: hip.hipMemsetAsync(buf.data_ptr(), 0xA5, buf.numel() * buf.element_size(), None)

    # 1. the image form
    frames, w, h, iq = 1000, 1920, 1080, 256
    ip = fsea.Interp(np.uint8, 2 * iq * iq)
    ip.push(rng.integers(0, 256, 2 * iq * iq, dtype=np.uint8))
    ip.push(rng.integers(0, 256, 2 * iq * iq, dtype=np.uint8))
    d_w = torch.tensor([R.sine_ease_in_out((f % 100) * 0.01) for f in range(frames)], dtype=torch.float64, device="cuda")
    out = torch.empty(frames * w * h, dtype=torch.uint8, device="cuda")
    beside("image form, %d frames of %d x %d" % (frames, w, h), out.numel(),
           lambda: ip.image_frames_device(d_w.data_ptr(), frames, w, h, iq, out.data_ptr()), plain(out))
    del out
    ip.close()
    if "--image-only" in sys.argv[1:]:
        return

    # 2. the sample form
    for dtype, n in ((np.uint8, 262144), (np.float64, 262144)):
        ip = fsea.Interp(dtype, n)
        for _ in range(2):
            ip.push(rng.integers(0, 256, n, dtype=np.uint8) if dtype == np.uint8 else rng.standard_normal(n))
        out = torch.empty(128 * n * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
        beside("sample form, 128 frames of %d %s" % (n, np.dtype(dtype).name), out.numel(),
               lambda: ip.frames_device(d_w.data_ptr(), 128, out.data_ptr()), plain(out))
        if dtype == np.uint8:
            one = ratelib.per_round(lambda: ip.frames_device(d_w.data_ptr(), 1, out.data_ptr()), WARMUP, REPS, ROUNDS)
            host = np.empty(n, dtype=np.uint8)
            dl = ratelib.wall(lambda: fsea._check(ip._L.fsea_copy_to_host(0, host.ctypes.data, out.data_ptr(), n)), 0, 20)
        del out
        ip.close()

    # 3. one nrf_interpolator_get_buffer call
    L = nrf.nrf_lib()
    a, b = rng.integers(0, 256, 262144, dtype=np.uint8), rng.integers(0, 256, 262144, dtype=np.uint8)
    itp = L.nrf_interpolator_new(0.01)
    for blk in (a, a, b):
        buf = L.nut_buffer_new_u8(131072, 2, blk.ctypes.data)
        L.nrf_interpolator_process(itp, buf)
        L.nut_buffer_free(buf)
    wall = []                  # not ratelib.wall: the buffer a call returns is freed outside the clock, before the next call
    for _ in range(60):
        t0 = time.perf_counter()
        got = L.nrf_interpolator_get_buffer(itp)
        wall.append(time.perf_counter() - t0)
        L.nut_buffer_free(got)
    L.nrf_interpolator_free(itp)
    ref = ratelib.wall(lambda: R.blend_frames(a, b, [0.01]), 0, 10)
    print("nrf_interpolator_get_buffer, 262144 U8: median wall %.1f us (min %.1f); one-frame launch %.1f us (events, best of "
          "%d rounds of %d); download of the frame %.1f us (median wall); restated host loop (numpy, one CPU) %.1f us (median)" %
          (statistics.median(wall[10:]) * 1e6, min(wall) * 1e6, min(one) * 1e6, ROUNDS, REPS, statistics.median(dl) * 1e6,
           statistics.median(ref) * 1e6))


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:]):
        run()


if __name__ == "__main__":
    main()
