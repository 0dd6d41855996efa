#!/usr/bin/env python3
"""Rates of the audio decoder (fsea_demod_*: fsea_demod_stage1_u8, fsea_demod_fm, fsea_demod_deemph, include/fsea.h).

1. nrf_decoder_process (WBFM, 5 MHz -> 48 kHz, offset 50000) on the replay block of 131072 pairs: median wall time of
   the call (host form: upload, three kernels, download, phase bookkeeping) against the 16.7 ms block period of the
   60 Hz replay.
2. The device form on 131072-pair blocks at 10 MHz, WBFM, K = 1, 8, 64, 256 channels with distinct offsets: time per
   call by HIP events (torch.cuda.Event around REPS calls on the null stream, best of ROUNDS), channel-samples/s, and the
   fraction of the binding bound max(input bytes / 8 TB/s, counted f64 FLOP / FP64 peak).  The FP64 peak is the
   measured v_fma_f64 rate of scripts/ubench/fp64_fma.hip, passed as --fp64-tflops; without it the fraction is not
   printed.  Counted FLOP per channel and input sample (FMA = 2, a divide = 1): conversion 4, rotation 6, phase
   recurrence 6, stage 1 (2 x 51 taps x 2) / rate_mul1, discriminator 20 / rate_mul1, stage 3 (41 x 2) / (rate_mul1
   rate_mul3), de-emphasis 3 / (rate_mul1 rate_mul3).
The measurement is one part, `run`, which also writes what it prints to profiles/demod_rate.txt (--out FILE: there
instead); without `run` on the command line it runs as a child process under its time limit.
Usage: python scripts/demod_rate.py [run] [--device-only] [--fp64-tflops X] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea, nrf  # noqa: E402
import ratelib  # noqa: E402

PAIRS = 131072
WARMUP, REPS, ROUNDS = 3, 20, 3
HBM_BPS = 8e12
CHANNELS = [1, 8, 64, 256]
# the part's time limit: three times its wall time on an MI355X (1.9 s), rounded up to 30 s, and at least 120 s -- a first
# import of torch on a fresh machine alone can take over a minute
STEP_LIMIT_S = 120


def flop_per_sample(in_rate, out_rate=48000):
    r1 = in_rate / 336000.0
    r3 = 336000.0 / out_rate
    return 4 + 6 + 6 + 2 * 51 * 2 / r1 + 20 / r1 + 41 * 2 / (r1 * r3) + 3 / (r1 * r3)


def block():
    with np.load(os.path.join(ROOT, "tests", "golden", "demod_golden.npz")) as z:
        return np.ascontiguousarray(z["block__raw"])


def host_call(lines):
    L = nrf.nrf_lib()
    samples = np.ascontiguousarray(block() ^ 0x80)
    dec = L.nrf_decoder_new(nrf.NRF_DEMODULATE_WBFM, 5000000, 48000, 50000)
    walls = ratelib.wall(lambda: L.nrf_decoder_process(dec, samples.ctypes.data, PAIRS), WARMUP, 100)
    L.nrf_decoder_free(dec)
    med = statistics.median(walls)
    lines.append("1. nrf_decoder_process, WBFM 5 MHz -> 48 kHz, 131072 pairs (host form), 100 calls")
    lines.append("  wall median %8.1f us (min %8.1f)   = %.3f of the 16.7 ms block period at 60 Hz"
                 % (med * 1e6, min(walls) * 1e6, med / (1 / 60.0)))


def device_calls(lines, fp64_tflops):
    import torch
    rate = 10000000
    raw = block()
    d_iq = torch.from_numpy(raw.copy()).to("cuda")
    flop = flop_per_sample(rate)
    lines.append("2. device form, WBFM 10 MHz -> 48 kHz, 131072 pairs per call (raw int8, flip), HIP events, best of %d x %d calls"
                 % (ROUNDS, REPS))
    lines.append("  counted f64 FLOP per channel-sample %.1f; FP64 peak %s" %
                 (flop, ("%.1f TFLOP/s (measured, scripts/ubench/fp64_fma.hip)" % fp64_tflops) if fp64_tflops else "unmeasured"))
    for K in CHANNELS:
        d = fsea.Demod("wbfm", rate, n_channels=K)
        for ch in range(K):
            d.set_channel(ch, -4800000 + 37500 * ch)
        out = torch.empty((K, d.out_length(PAIRS)), dtype=torch.float64, device="cuda")

        def call():
            d.run_device(d_iq.data_ptr(), PAIRS, out.data_ptr(), flip=True)

        best = min(ratelib.per_round(call, WARMUP, REPS, ROUNDS))
        d.close()
        cs = K * PAIRS / best
        t_bytes = 2 * PAIRS / HBM_BPS
        line = "  K=%3d  %9.1f us per call  %8.3f G channel-samples/s  %7.2f TFLOP/s counted" % (
            K, best * 1e6, cs / 1e9, cs * flop / 1e12)
        if fp64_tflops:
            t_flop = K * PAIRS * flop / (fp64_tflops * 1e12)
            bound = max(t_bytes, t_flop)
            line += "  bound %s %.2f us  fraction %.3f" % ("FP64" if t_flop >= t_bytes else "HBM", bound * 1e6, bound / best)
        lines.append(line)


def run():
    import torch
    torch.cuda.init()     # torch's HIP runtime first, then the libraries (libfsea_hip.so loaded globally, as the tests do)
    fsea.hip_lib()
    ap = argparse.ArgumentParser()
    ap.add_argument("run")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--fp64-tflops", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demod_rate.txt"))
    a = ap.parse_args()
    lines = ["# scripts/demod_rate.py on one MI355X (fsea_demod_stage1_u8 + fsea_demod_fm + fsea_demod_deemph)"]
    if not a.device_only:
        host_call(lines)
    device_calls(lines, a.fp64_tflops)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fp:
        fp.write(text)


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:]):
        run()


if __name__ == "__main__":
    main()
