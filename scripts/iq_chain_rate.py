#!/usr/bin/env python3
"""What the IQ chain (nrf_iq_chain, fsea_chain_*, kernel fsea_shift_fir_u8) buys, in two parts.

percall: one 131072-pair u8 block per call, median wall time of nrf_iq_chain against the block sequence it replaces, both in
         this process on this build --
           dvbt:   nrf_freq_shifter -> nrf_iq_filter(5e6, 60e3, 97) -> nrf_buffer_to_iq_points   (lua/dvbt.lua:46-51)
           iq-tex: nrf_iq_filter(5e6, 200e3, 51) -> nrf_buffer_to_iq_lines(4, 0.2)               (lua/iq-tex-filtered.lua:44-47)
         every buffer freed as the scene's garbage collector would.
kernel:  the shifted FIR kernel against the unshifted one at n = 2^26, L = 21, 51, 97, with scripts/fir_roofline.py's method
         and bound (the rotation's flops are not algorithmic work).

Without an argument both parts run, each as a child process under its own time limit; a part that fails ends the run.
Usage: python scripts/iq_chain_rate.py [percall|kernel] [--to FILE]   (--to: what the parts print goes there too)"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea, nrf  # noqa: E402
import ratelib  # noqa: E402

PAIRS = 131072
WARMUP_CALLS, CALLS = 30, 300
N = 1 << 26
WARMUP, REPS, ROUNDS = 5, 20, 5
HBM_BPS, VALU_FLOPS = 8e12, 157.3e12
STEP_LIMIT_S = {"percall": 240, "kernel": 240}


def percall():
    L = nrf.nrf_lib()
    block = np.random.default_rng(2).integers(0, 256, 2 * PAIRS, dtype=np.uint8)
    buf = L.nut_buffer_new_u8(PAIRS, 2, block.ctypes.data)
    print("one %d-pair u8 block per call, median (min) wall time of %d calls after %d" % (PAIRS, CALLS, WARMUP_CALLS))

    def scene(name, shift, cutoff, taps, draw_blocks, draw_chain):
        shifter = L.nrf_freq_shifter_new(shift, 5000000) if shift else None
        flt = L.nrf_iq_filter_new(5000000, cutoff, taps)
        chain = L.nrf_iq_chain_new(5000000, cutoff, taps)
        if shift:
            L.nrf_iq_chain_set_shifter(chain, shift)

        def blocks():
            src, sb = buf, None
            if shifter:
                L.nrf_freq_shifter_process(shifter, buf)
                src = sb = L.nrf_freq_shifter_get_buffer(shifter)
            L.nrf_iq_filter_process(flt, src)
            fb = L.nrf_iq_filter_get_buffer(flt)
            L.nut_buffer_free(draw_blocks(fb))
            L.nut_buffer_free(fb)
            if sb:
                L.nut_buffer_free(sb)

        def chained():
            L.nrf_iq_chain_process(chain, buf)
            L.nut_buffer_free(draw_chain(chain))

        # both end in the draw's download of its image: the wall time of a call holds all of its work
        b, c = ([t * 1e6 for t in ratelib.median_min(ratelib.wall(fn, WARMUP_CALLS, CALLS))] for fn in (blocks, chained))
        print("%-7s block sequence %8.1f us (%8.1f)   nrf_iq_chain %7.1f us (%7.1f)   ratio %.2f"
              % (name, b[0], b[1], c[0], c[1], b[0] / c[0]))
        L.nrf_iq_chain_free(chain)
        L.nrf_iq_filter_free(flt)
        if shifter:
            L.nrf_freq_shifter_free(shifter)
        return b[0] > c[0]

    ok = scene("dvbt", 50000, 60000, 97, L.nrf_buffer_to_iq_points, L.nrf_iq_chain_get_iq_points)
    ok &= scene("iq-tex", 0, 200000, 51, lambda fb: L.nrf_buffer_to_iq_lines(fb, 4, 0.2),
                lambda ch: L.nrf_iq_chain_get_iq_lines(ch, 4, 0.2))
    L.nut_buffer_free(buf)
    if not ok:
        raise SystemExit("the chain's median is not below the block sequence's")


def kernel():
    import torch
    L = fsea.hip_lib()
    iq = np.random.default_rng(1).integers(0, 256, 2 * N, dtype=np.uint8)
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    fsea._check(L.fsea_device_alloc(0, iq.nbytes, ctypes.byref(d_in)))
    fsea._check(L.fsea_device_alloc(0, 8 * N, ctypes.byref(d_out)))
    fsea._check(L.fsea_copy_to_device(0, d_in, iq.ctypes.data, iq.nbytes))
    torch.cuda.init()
    print("n = %d samples, u8 -> f32 complex, %d launches per timing, best of %d" % (N, REPS, ROUNDS))
    for taps in (21, 51, 97):
        fir = fsea.Fir(fsea.lowpass_taps(5e6, 200e3, taps))
        launches = (("fsea_fir_u8", lambda: fir.run_device(d_in.value, N, d_out.value, flip=True)),
                    ("fsea_shift_fir_u8", lambda: fir.run_shifted_device(d_in.value, N, d_out.value, 50e3 / 5e6, 0.0, 0, flip=True)),
                    ("fsea_shift_fir_u8 +3", lambda: fir.run_shifted_device(d_in.value, N, d_out.value, 50e3 / 5e6, 0.0, 3,
                                                                             flip=True)))
        bound = max(10.0 * N / HBM_BPS, 4.0 * taps * N / VALU_FLOPS)
        for name, launch in launches:      # "+3": a call that starts off the 8-sample grid (two phasor bases per group)
            best = min(ratelib.per_round(launch, WARMUP, REPS, ROUNDS))
            print("L=%-3d %-21s achieved %8.1f us   bound %8.1f us   fraction %.3f" % (taps, name, best * 1e6, bound * 1e6,
                                                                                     bound / best))
        fir.close()
    fsea._check(L.fsea_device_free(0, d_in))
    fsea._check(L.fsea_device_free(0, d_out))


def main():
    part = ratelib.run_parts(__file__, STEP_LIMIT_S, sys.argv[1:])
    if part:
        {"percall": percall, "kernel": kernel}[part]()


if __name__ == "__main__":
    main()
