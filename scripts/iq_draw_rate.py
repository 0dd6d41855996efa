#!/usr/bin/env python3
"""Rates of the IQ constellation kernels (fsea_iq_points_* and fsea_iq_lines_* + fsea_iq_clamp, include/fsea.h).

1. Per call, one frame on the host (what a scene pays each frame): nrf_buffer_to_iq_points and
   nrf_buffer_to_iq_lines(buf, 4, 0.3) on the F64 output of nrf_iq_filter (5 MHz, 200 kHz, 51 taps) of the replay block:
   median wall time of the nrf call, and its parts measured alone with HIP events -- upload (pinned -> device, 2 MiB),
   kernels (the device form on that frame), download (the image, device -> pinned).
2. Batched, device-resident: 512 frames of 131072 u8 pairs.  points: pairs/s and the fraction of the 8 TB/s HBM roofline
   by bytes read (2 per pair) + written (65536 per frame); lines (m = 1 and 4, 0.3 of the points): pixel increments/s
   (sum over segments of max(dx, dy) + 1, counted on the host over every 64th frame and scaled by 64).  Inputs: the
   replay block, the sixteen short captures (both recorded: tests/golden/rfdata_all_golden.npz), and uniform random bytes.
HIP events (torch.cuda.Event on the null stream, where the launches go) around REPS launches after WARMUP, best of ROUNDS.
The measurement is one part, `run`; without it on the command line it runs as a child process under its time limit.
Usage: python scripts/iq_draw_rate.py [run] [--batched-only] [block|captures|random ...] [--to FILE]   (default: 1. and 2.,
every input; a counters run per input takes one input name and names the part, `run --batched-only random`, so that the
profiler's child is the process that measures)"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea, nrf  # noqa: E402
import ratelib  # noqa: E402

FRAMES, PAIRS = 512, 131072
WARMUP, REPS, ROUNDS = 2, 5, 3
# the part's time limit: three times its wall time on an MI355X (7.0 s), rounded up to 30 s, and at least 120 s -- a first
# import of torch on a fresh machine alone can take over a minute
STEP_LIMIT_S = 120
HBM_BPS = 8e12


def best(fn, reps=REPS):
    return min(ratelib.per_round(fn, WARMUP, reps, ROUNDS))


def increments(iq_u8, m, n_points):
    c = iq_u8.astype(np.int64)
    x, y = c[0:2 * n_points:2] * m, c[1:2 * n_points:2] * m
    return int((np.maximum(np.abs(np.diff(x)), np.abs(np.diff(y))) + 1).sum())


def per_call(L, draw, torch):
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        block = np.ascontiguousarray(z["block__raw"] ^ 0x80)
    flt = L.nrf_iq_filter_new(5000000, 200000, 51)
    buf = L.nut_buffer_new_u8(block.size // 2, 2, block.ctypes.data)
    L.nrf_iq_filter_process(flt, buf)
    fb = L.nrf_iq_filter_get_buffer(flt)
    f64 = nrf.buffer_to_numpy(L, fb)
    n = f64.size // 2
    n_points = (int(np.float32(f64.size) * np.float32(0.3)) + 1) // 2
    print("1. per call, one frame: nrf_iq_filter(5e6, 200e3, 51) output of the replay block, F64, %d pairs" % n)
    calls = {"points": lambda: L.nut_buffer_free(L.nrf_buffer_to_iq_points(fb)),
             "lines m=4 0.3": lambda: L.nut_buffer_free(L.nrf_buffer_to_iq_lines(fb, 4, 0.3))}
    h_in = torch.from_numpy(f64).pin_memory()
    d_in = h_in.to("cuda")
    for name, fn in calls.items():
        walls = ratelib.wall(fn, 3, 20)
        m = 4 if name.startswith("lines") else 1
        img_bytes = (256 * m) ** 2
        d_img = torch.empty(img_bytes, dtype=torch.uint8, device="cuda")
        h_img = torch.empty(img_bytes, dtype=torch.uint8).pin_memory()
        up = best(lambda: d_in.copy_(h_in, non_blocking=True))
        if m == 1:
            k = best(lambda: draw.points_device(d_in.data_ptr(), fsea.IQ_F64, n, 1, d_img.data_ptr()))
        else:
            k = best(lambda: draw.lines_device(d_in.data_ptr(), fsea.IQ_F64, n_points, 1, 4, d_img.data_ptr()))
        down = best(lambda: h_img.copy_(d_img, non_blocking=True))
        print("  %-14s wall median %7.1f us (min %7.1f)   upload %6.1f us (%d B)   kernels %7.1f us   download %6.1f us (%d B)"
              % (name, statistics.median(walls) * 1e6, min(walls) * 1e6, up * 1e6, f64.nbytes, k * 1e6, down * 1e6,
                 img_bytes))
    L.nut_buffer_free(fb)
    L.nut_buffer_free(buf)
    L.nrf_iq_filter_free(flt)


def batched(draw, torch, names):
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        block = z["block__raw"] ^ 0x80
        caps = np.concatenate([z[k] for k in sorted(z.files) if k.endswith("__raw") and k.startswith("rf_")][:16]) ^ 0x80
    inputs = {"replay block": lambda: np.tile(block, FRAMES), "16 captures": lambda: np.tile(caps, FRAMES),
              "uniform random": lambda: np.random.default_rng(1).integers(0, 256, 2 * PAIRS * FRAMES, dtype=np.uint8)}
    inputs = {k: v for k, v in inputs.items() if not names or k.split()[-1] in names}
    print("2. batched, device-resident: %d frames x %d u8 pairs" % (FRAMES, PAIRS))
    for name, make in inputs.items():
        iq = make()
        d_in = torch.from_numpy(iq).to("cuda")
        d_pts = torch.empty(FRAMES * 65536, dtype=torch.uint8, device="cuda")
        t = best(lambda: draw.points_device(d_in.data_ptr(), fsea.IQ_U8, PAIRS, FRAMES, d_pts.data_ptr()))
        nbytes = 2.0 * PAIRS * FRAMES + 65536.0 * FRAMES
        print("  %-15s points      %8.1f us  %7.2f Gpairs/s  %7.1f GB/s  fraction of HBM roofline %.3f"
              % (name, t * 1e6, PAIRS * FRAMES / t / 1e9, nbytes / t / 1e9, nbytes / HBM_BPS / t))
        del d_pts
        for m in (1, 4):
            n_points = (int(np.float32(2 * PAIRS) * np.float32(0.3)) + 1) // 2
            inc = sum(increments(iq[f * 2 * PAIRS:(f + 1) * 2 * PAIRS], m, n_points) for f in range(0, FRAMES, 64)) * 64
            d_img = torch.empty(FRAMES * (256 * m) ** 2, dtype=torch.uint8, device="cuda")
            t = best(lambda: draw.lines_device(d_in.data_ptr(), fsea.IQ_U8, n_points, FRAMES, m, d_img.data_ptr()),
                      reps=2)
            print("  %-15s lines m=%d   %8.1f us  %7.2f G pixel increments/s  (%.3g increments, %d points per frame)"
                  % (name, m, t * 1e6, inc / t / 1e9, inc, n_points))
            del d_img
        del d_in
        torch.cuda.empty_cache()


def run():
    import torch
    torch.cuda.init()
    L = nrf.nrf_lib()
    draw = fsea.IqDraw()
    args = [a for a in sys.argv[1:] if a != "run"]
    if "--batched-only" not in args:
        per_call(L, draw, torch)
    batched(draw, torch, [a for a in args if not a.startswith("--")])
    draw.close()


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:]):
        run()


if __name__ == "__main__":
    main()
