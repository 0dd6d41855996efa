#!/usr/bin/env python3
"""Rate of the burst detector (fsea_detect_u8_device, include/fsea.h) beside a plain read-only stream.

The detector reads every byte of a recording and writes 24 bytes per block: its rate is bytes read per second.  Two shapes
of 1 GiB each, four times the Infinity Cache: 4096 blocks of 262144 bytes (the scene's block; kernel fsea_detect_slices)
and 262144 blocks of 4096 bytes (kernel fsea_detect_waves).  Each is timed with HIP events on the null stream around REPS
launches after a warm-up, ROUNDS rounds, twice; printed: every round's time and the best.  Before, between and after them
the read-only kernel of scripts/ubench/stream_rw.hip runs as a program of its own on the same card (built on first use; it
takes the best of five launches per grid): the plain stream the detector is measured against.  The ratio printed is
detector rate over the best read-only rate.  The stream runs in a process of its own, with its own allocation and clock
history, and its figure is the best over three grids and three runs: the ratio compares two bests taken seconds apart on
one card and moves with the clock state by a few per cent.  The registers of the kernels are read from the shipped code object.
The measurement is one part, `run`; without it on the command line it runs as a child process under its time limit.
Usage: python scripts/detect_rate.py [run] [--launch-only] [--to FILE]   (--launch-only: the detector alone; a trace or
counters run names the part, `run --launch-only`, so that the profiler's child is the process that measures)"""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

WARMUP, REPS, ROUNDS = 20, 3, 5   # 20 launches of 1 GiB settle the clocks before the first timed round
# the part's time limit: three times its wall time on an MI355X (3.3 s), rounded up to 30 s, and at least 120 s -- a first
# import of torch on a fresh machine alone can take over a minute
STEP_LIMIT_S = 120
SHAPES = [(4096, 262144), (262144, 4096)]
STREAM_SRC = os.path.join(ROOT, "scripts", "ubench", "stream_rw.hip")
STREAM = os.path.join(ROOT, "scripts", "ubench", "bin", "stream_rw")


def read_only_stream():
    """GB/s of stream_rw's read-only kernel, one figure per grid it tries."""
    if not os.path.exists(STREAM):
        os.makedirs(os.path.dirname(STREAM), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", STREAM_SRC, "-o", STREAM],
                       check=True)
    text = subprocess.run([STREAM], check=True, capture_output=True, text=True).stdout
    return [float(m) for m in re.findall(r"read only\s+[\d.]+ ms\s+(\d+) GB/s", text)]


def run():
    import torch
    from tests.test_shipped_artifacts import _kernels
    if fsea.device_count() < 1:
        sys.exit("detect_rate.py needs a GPU")
    launch_only = "--launch-only" in sys.argv[1:]
    ks = _kernels(fsea.lib_path())
    for name in sorted(k for k in ks if k.startswith("fsea_detect_")):
        k = ks[name]
        print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch" %
              (name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]))
    nbytes = SHAPES[0][0] * SHAPES[0][1]
    rng = np.random.default_rng(1)
    data = torch.from_numpy(np.tile(rng.integers(0, 256, 1 << 24, dtype=np.uint8), nbytes >> 24)).cuda()
    sums = torch.empty(3 * max(n for n, _ in SHAPES), dtype=torch.int64, device="cuda")
    det = fsea.Detect()
    plain = [] if launch_only else read_only_stream()
    best = {}
    for _ in range(2):
        for n_blocks, block_bytes in SHAPES:
            assert n_blocks * block_bytes == nbytes
            ts = ratelib.per_round(lambda: det.sums_device(data.data_ptr(), block_bytes, n_blocks, sums.data_ptr()), WARMUP, REPS, ROUNDS)
            print("%d blocks x %d bytes, ms: %s" % (n_blocks, block_bytes, " ".join("%.3f" % (t * 1e3) for t in ts)))
            best[(n_blocks, block_bytes)] = min(ts + [best.get((n_blocks, block_bytes), 1e9)])
        if not launch_only:
            plain += read_only_stream()
    det.close()
    for (n_blocks, block_bytes), t in best.items():
        line = "detector, %d blocks x %d bytes: best %.3f ms = %.0f GB/s read" % (n_blocks, block_bytes, t * 1e3, nbytes / t / 1e9)
        if plain:
            line += "; %.3f of the read-only stream" % (nbytes / t / 1e9 / max(plain))
        print(line)
    if plain:
        print("read-only stream (scripts/ubench/stream_rw.hip, 1 GiB, best of 5 per grid), GB/s: %s; best %.0f" %
              (" ".join("%.0f" % p for p in plain), max(plain)))


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:]):
        run()


if __name__ == "__main__":
    main()
