#!/usr/bin/env python3
"""Rate of the IQ trace movie (fsea_trace_frames_device, include/fsea.h) beside a plain store stream.

1. The movie launch at the tool's geometry: 1000 frames of 1920 x 1080 from 100 bytes each (the tool's defaults), and
   from 1024 bytes each with -f 3 -p 40 (u32 counts, a canvas that fills), in one call each (2.07 GB written).  Beside
   each, in the same process, hipMemsetAsync of the same byte count on the same buffer: the plain store stream the launch
   is measured against.  The two are timed alternately, HIP events on the null stream around REPS launches after a
   warm-up, ROUNDS rounds; printed: every round's time, the best, and launch over plain stream of the bests.  The
   launch's parts (zeroing the count planes, hit pass, compose pass) are in a kernel trace of this script, not here.
2. The tool on one 262144-byte capture at its defaults (2622 frames): wall time with --raw and as PNG files, and the time
   write_gray_png alone takes for the same frames (the share that is PNG encoding).
The registers of the kernels are read from the shipped code object.
The measurement is one part, `run`; without it on the command line it runs as a child process under its time limit.
Usage: python scripts/trace_rate.py [run] [--launch-only] [--to FILE]   (--launch-only: 1. alone; a trace or counters run
names the part, `run --launch-only`, so that the profiler's child is the process that measures)"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea, nrf  # noqa: E402
import ratelib  # noqa: E402

WARMUP, REPS, ROUNDS = 2, 3, 5
# the part's time limit: three times its wall time on an MI355X (7.7 s), rounded up to 30 s, and at least 120 s -- a first
# import of torch on a fresh machine alone can take over a minute
STEP_LIMIT_S = 120
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-single-sample")


def beside(name, nbytes, kernel, plain):
    k, p = [], []
    for _ in range(2):                       # alternately
        k += ratelib.per_round(kernel, WARMUP, REPS, ROUNDS)
        p += ratelib.per_round(plain, WARMUP, REPS, ROUNDS)
    fmt = lambda ts: " ".join("%.3f" % (t * 1e3) for t in ts)
    print("%s: %.1f MB written per launch" % (name, nbytes / 1e6))
    print("  movie launch ms: %s   best %.3f ms = %.0f GB/s" % (fmt(k), min(k) * 1e3, nbytes / min(k) / 1e9))
    print("  plain stream ms: %s   best %.3f ms = %.0f GB/s" % (fmt(p), min(p) * 1e3, nbytes / min(p) / 1e9))
    print("  movie time / plain-stream time (bests): %.3f; plain-stream spread %.1f %%" %
          (min(k) / min(p), 100 * (max(p) - min(p)) / min(p)))


def run():
    import torch
    from tests.test_shipped_artifacts import _kernels
    if fsea.device_count() < 1:
        sys.exit("trace_rate.py needs a GPU")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    ks = _kernels(fsea.lib_path())
    for name in sorted(k for k in ks if k.startswith("fsea_trace_")):
        k = ks[name]
        print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch" %
              (name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]))
    rng = np.random.default_rng(1)

    # 1. the movie launch
    frames, w, h = 1000, 1920, 1080
    out = torch.empty(frames * w * h, dtype=torch.uint8, device="cuda")
    plain = lambda: hip.hipMemsetAsync(out.data_ptr(), 0xA5, out.numel(), None)
    for s, p, f in ((100, 4, 0), (1024, 40, 3)):
        data = torch.from_numpy(rng.normal(0, 40, frames * s).clip(-128, 127).astype(np.int8).view(np.uint8)).cuda()
        tr = fsea.Trace(w, h, 4, p, f)
        beside("movie, %d frames of %d x %d, -s %d -p %d -f %d" % (frames, w, h, s, p, f), out.numel(),
               lambda: tr.frames_device(data.data_ptr(), data.numel(), s, frames, out.data_ptr()), plain)
        tr.close()
    del out
    if "--launch-only" in sys.argv[1:]:
        return

    # 2. the tool on one capture
    L = nrf.nrf_lib()
    L.write_gray_png.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    capture = rng.normal(0, 40, 262144).clip(-128, 127).astype(np.int8).view(np.uint8)
    n = 262144 // 100 + 1
    with tempfile.TemporaryDirectory() as tmp:
        capture.tofile(os.path.join(tmp, "capture.raw"))
        wall = {}
        for mode in ("raw", "png"):
            os.makedirs(os.path.join(tmp, mode))
            t0 = time.perf_counter()
            subprocess.run([TOOL, "--out", os.path.join(tmp, mode)] + (["--raw"] if mode == "raw" else []) +
                           [os.path.join(tmp, "capture.raw")], check=True, stdout=subprocess.DEVNULL)
            wall[mode] = time.perf_counter() - t0
        # the encoder alone on the same frames, read back from the raw run
        enc = 0.0
        for no in range(1, n + 1, 20):
            img = np.fromfile(os.path.join(tmp, "raw", "sample-%d.raw" % no), dtype=np.uint8)
            t0 = time.perf_counter()
            L.write_gray_png(os.path.join(tmp, "enc.png").encode(), w, h, img.ctypes.data)
            enc += time.perf_counter() - t0
        enc *= n / len(range(1, n + 1, 20))
    print("fsea-single-sample, one 262144-byte capture, %d frames: --raw %.2f s wall, PNG %.2f s wall; write_gray_png alone on "
          "these frames %.2f s (every 20th frame timed, scaled) = %.0f %% of the PNG run" %
          (n, wall["raw"], wall["png"], enc, 100 * enc / wall["png"]))


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:]):
        run()


if __name__ == "__main__":
    main()
