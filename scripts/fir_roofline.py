#!/usr/bin/env python3
"""Achieved time of the streaming FIR kernel (fsea_fir_u8_device: u8 IQ in, f32 complex out, device-resident) against its
roofline bound per launch, max(bytes / 8 TB/s, 4 L n / 157.3 TFLOP/s), bytes = 2 read + 8 written per sample.  HIP events
(torch.cuda.Event on the null stream, where the launches go) around REPS back-to-back launches after WARMUP.
The measurement is one part, `run`; without it on the command line it runs as a child process under its time limit.
Usage: python scripts/fir_roofline.py [run] [L ...] [--to FILE]        (default 21 51 97; n = 2^26 samples)"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N = 1 << 26
WARMUP, REPS, ROUNDS = 5, 20, 5
HBM_BPS, VALU_FLOPS = 8e12, 157.3e12
# the part's time limit: three times its wall time on an MI355X (2.2 s), rounded up to 30 s, and at least 120 s -- a first
# import of torch on a fresh machine alone can take over a minute
STEP_LIMIT_S = 120


def run():
    import torch
    lengths = [int(a) for a in sys.argv[1:] if a != "run"] or [21, 51, 97]
    L = fsea.hip_lib()
    iq = np.random.default_rng(1).integers(0, 256, 2 * N, dtype=np.uint8)
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    fsea._check(L.fsea_device_alloc(0, iq.nbytes, ctypes.byref(d_in)))
    fsea._check(L.fsea_device_alloc(0, 8 * N, ctypes.byref(d_out)))
    fsea._check(L.fsea_copy_to_device(0, d_in, iq.ctypes.data, iq.nbytes))
    torch.cuda.init()
    print("n = %d samples, u8 -> f32 complex, %d launches per timing, best of %d" % (N, REPS, ROUNDS))
    for taps in lengths:
        fir = fsea.Fir(fsea.lowpass_taps(5e6, 200e3, taps))
        best = min(ratelib.per_round(lambda: fir.run_device(d_in.value, N, d_out.value, flip=True), WARMUP, REPS, ROUNDS))
        t_hbm = 10.0 * N / HBM_BPS
        t_valu = 4.0 * taps * N / VALU_FLOPS
        bound = max(t_hbm, t_valu)
        print("L=%-3d achieved %8.1f us   bound %8.1f us (%s; HBM %.1f us, VALU %.1f us)   fraction %.3f   %6.1f GB/s  %6.1f TFLOP/s"
              % (taps, best * 1e6, bound * 1e6, "compute" if t_valu > t_hbm else "HBM", t_hbm * 1e6, t_valu * 1e6,
                 bound / best, 10.0 * N / best / 1e9, 4.0 * taps * N / best / 1e12))
        fir.close()
    fsea._check(L.fsea_device_free(0, d_in))
    fsea._check(L.fsea_device_free(0, d_out))


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:]):
        run()


if __name__ == "__main__":
    main()
