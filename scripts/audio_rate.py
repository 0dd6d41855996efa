#!/usr/bin/env python3
"""What the audio of a table of cut-outs (fsea_audio_*, kernel fsea_audio_tiles) costs against the extract call that made the
pairs and against one call per cut-out, on a resident recording of 2^25 samples, L = 97, D = 4, 16, 64; FM, 41 audio taps,
D2 = 2.  HIP-event times in one process, median of REPS calls after WARMUP:

(a) one fsea_audio_run_device of 256 jobs of 65536 / D pairs each on the pairs (c) left, the jobs at even and odd firsts in
    turn;
(b) 256 fsea_audio_run_device calls of one job each: the route of a caller that demodulates cut-out by cut-out;
(c) the fsea_extract_run_device call that made those pairs: 256 jobs of 65536 + D samples, as scripts/extract_rate.py lays
    them over the recording.

Two bounds for (a): 8 bytes per pair in and 4 / D2 out at 8 TB/s, and the counted f64 instructions per pair -- the discriminator
(2 conversions, 2 subtractions, 6 for the two products, about 40 for two divisions as the compiler expands them, 5 for the
polynomial, the angle and the sign) and the chain (2 L2 / D2) -- against the 32.9 T f64 instructions a second behind the 65.8
TFLOP/s that scripts/ubench/fp64_fma.hip measured (an FMA counts 2).

`trace` runs TRACE_CALLS calls of (a) at D = 16 in a child of its own under a kernel trace (nothing else traced) and prints the
median time of each of the two kernels of a call.

Without an argument every D and then the trace run as child processes under their own time limits and the lines go to
profiles/audio_rate.txt (or the file named after --to); a part that fails ends the run.
Usage: python scripts/audio_rate.py [--to FILE] | python scripts/audio_rate.py measure D | ... trace      (D = 4, 16 or 64)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N_SAMPLES = 1 << 25
TAPS = 97
DECIMATIONS = (4, 16, 64)
AUDIO_TAPS, AUDIO_D = 41, 2
N_JOBS, JOB_BASE = 256, 65536
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
F64_OPS_PER_PAIR = 2 + 2 + 6 + 40 + 5 + 2 * AUDIO_TAPS // AUDIO_D
F64_OPS_PER_S = 65.8e12 / 2
STEP_LIMIT_S = 240
TRACE_D, TRACE_CALLS = 16, 10
KERNELS = ("fsea_jobs_upload", "fsea_audio_tiles")     # a call's two, in launch order

HEADER = """# scripts/audio_rate.py on one MI355X: HIP-event times in one process, median (min) of %d calls after %d
# recording: 2^25 samples resident, L = %d, taps = lowpass(10e6, 10e6 / (2 D), %d); FM, %d audio taps, D2 = %d, offset (0.5 + 0.5j) sum(c)
# (a) one fsea_audio_run_device: %d jobs of 65536 / D pairs on the pairs of (c), first_pair = out_first + i mod 2
# (b) %d fsea_audio_run_device calls of one job each
# (c) the fsea_extract_run_device that made the pairs: %d jobs of 65536 + D samples, first = 131072 i + 3 + i mod 5, a centre per job
# traffic bound = 8 bytes per pair in, 4 / D2 out at 8 TB/s; f64 bound = %d instructions per pair at 32.9 T/s (65.8 TFLOP/s of v_fma_f64, FMA = 2)
# host time: wall time of the call (a) itself, until it returns
""" % (REPS, WARMUP, TAPS, TAPS, AUDIO_TAPS, AUDIO_D, N_JOBS, N_JOBS, N_JOBS, F64_OPS_PER_PAIR)


def setup(D):
    """the three routes as calls, and what to release afterwards"""
    x = ratelib.cutouts(fsea, D, JOB_BASE + D, N_SAMPLES, TAPS, N_JOBS)
    pair_rate = 10e6 / D
    au = fsea.Audio("fm", fsea.lowpass_taps(pair_rate, 0.4 * pair_rate / AUDIO_D, AUDIO_TAPS), AUDIO_D)
    ajobs, n_audio = au.layout([fsea.AudioJob(j.out_first + i % 2, JOB_BASE // D, 0) for i, j in enumerate(x.table)])
    singles = [(fsea.AudioJob * 1)(j) for j in ajobs]
    d_audio = fsea.DeviceBuffer(4 * n_audio)
    gain = pair_rate / (2 * np.pi * 75000.0)

    def a():
        au.run_device(x.d_pairs.ptr.value, x.total, ajobs, d_audio.ptr.value, n_audio, offset=x.offset, gain=gain)

    def b():
        for one in singles:
            au.run_device(x.d_pairs.ptr.value, x.total, one, d_audio.ptr.value, n_audio, offset=x.offset, gain=gain)

    x.extract()
    return a, b, x.extract, (x.ex, au), (x.d_in, x.d_pairs, d_audio)


def measure(D):
    a, b, c_route, objects, buffers = setup(D)
    n_pairs = JOB_BASE // D
    (tc, tc_min), (ta, ta_min), (tb, tb_min) = (ratelib.median_min(ratelib.per_call(fn, WARMUP, REPS)) for fn in (c_route, a, b))
    # what the host spends inside the call (a) before it returns: checks, the table of 256 jobs, two launches
    sync = fsea.Plan(128)
    host = ratelib.host_time(a, sync.synchronize, REPS)
    sync.close()
    pairs = N_JOBS * n_pairs
    traffic, f64 = (8.0 + 4.0 / AUDIO_D) * pairs / HBM_BPS, F64_OPS_PER_PAIR * pairs / F64_OPS_PER_S
    print("D=%-2d %d pairs in %d jobs   (a) audio %8.1f us (%8.1f)   (b) %d one-job calls %9.1f us (%9.1f)   (c) the extract call %8.1f us (%8.1f)"
          "   traffic bound %5.2f us   f64 bound %5.2f us   (a)/(c) %.3f   (b)/(a) %.1f   host time of (a) %.1f us"
          % (D, pairs, N_JOBS, ta * 1e6, ta_min * 1e6, N_JOBS, tb * 1e6, tb_min * 1e6, tc * 1e6, tc_min * 1e6, traffic * 1e6, f64 * 1e6,
             ta / tc, tb / ta, float(np.median(host)) * 1e6))
    ratelib.release(objects, buffers)


def launches():
    """what the trace sees: TRACE_CALLS calls of (a) at TRACE_D"""
    a, b, c_route, objects, buffers = setup(TRACE_D)
    ratelib.traced_calls(fsea, a, TRACE_CALLS)
    ratelib.release(objects, buffers)


def trace():
    times = ratelib.call_kernel_times(__file__, KERNELS, "fsea_audio_", TRACE_CALLS)
    print("kernel trace, D=%d, %d calls of (a): " % (TRACE_D, TRACE_CALLS) +
          "   ".join("%s %.1f us" % (k, t * 1e6) for k, t in zip(KERNELS, times)))


def main():
    if sys.argv[1:] == ["launches"]:         # the traced child of `trace`, not a part of its own
        return launches()
    parts = {"measure %d" % D: STEP_LIMIT_S for D in DECIMATIONS}
    parts["trace"] = STEP_LIMIT_S
    part = ratelib.run_parts(__file__, parts, sys.argv[1:], to=os.path.join(ROOT, "profiles", "audio_rate.txt"), header=HEADER + "\n")
    if part == "trace":
        trace()
    elif part:
        measure(int(part.split()[1]))


if __name__ == "__main__":
    main()
