#!/usr/bin/env python3
"""What the moment sums of a table of cut-outs (fsea_measure_*, kernels fsea_measure_tiles and fsea_measure_fold) cost against
the extract call that made the pairs and against one call per cut-out, on a resident recording of 2^25 samples, L = 97,
D = 4, 16, 64.  HIP-event times in one process, median of REPS calls after WARMUP:

(a) one fsea_measure_run_device of 256 jobs of 65536 / D pairs each on the pairs (b) left, the jobs at even and odd firsts
    in turn, lag 1;
(b) the fsea_extract_run_device call that made those pairs: 256 jobs of 65536 + D samples, as scripts/extract_rate.py lays
    them over the recording;
(c) 256 fsea_measure_run_device calls of one job each: the route of a caller that measures cut-out by cut-out.

Two bounds for (a): 8 bytes per pair at 8 TB/s, and the counted f64 instructions per pair -- 4 conversions, 4 subtractions, 3
for P, 1 for Q, 6 for the two R terms, 6 accumulations, 1 comparison: 25, none of them fused -- against the 32.9 T f64
instructions a second behind the 65.8 TFLOP/s that scripts/ubench/fp64_fma.hip measured (an FMA counts 2).

`trace` runs TRACE_CALLS calls of (a) at D = 16 in a child of its own under a kernel trace (nothing else traced) and prints the
median time of each of the three kernels of a call.

Without an argument every D and then the trace run as child processes under their own time limits and the lines go to
profiles/measure_rate.txt (or the file named after --to); a part that fails ends the run.
Usage: python scripts/measure_rate.py [--to FILE] | python scripts/measure_rate.py measure D | ... trace      (D = 4, 16 or 64)"""
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
N_JOBS, JOB_BASE = 256, 65536
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
F64_OPS_PER_PAIR = 25
F64_OPS_PER_S = 65.8e12 / 2
STEP_LIMIT_S = 240
TRACE_D, TRACE_CALLS = 16, 10
KERNELS = ("fsea_jobs_upload", "fsea_measure_tiles", "fsea_measure_fold")     # a call's three, in launch order

HEADER = """# scripts/measure_rate.py on one MI355X: HIP-event times in one process, median (min) of %d calls after %d
# recording: 2^25 samples resident, L = %d, taps = lowpass(10e6, 10e6 / (2 D), %d); lag 1, offset (0.5 + 0.5j) sum(c)
# (a) one fsea_measure_run_device: %d jobs of 65536 / D pairs on the pairs of (b), first_pair = out_first + i mod 2
# (b) the fsea_extract_run_device that made them: %d jobs of 65536 + D samples, first = 131072 i + 3 + i mod 5, a centre per job
# (c) %d fsea_measure_run_device calls of one job each
# traffic bound = 8 bytes per pair at 8 TB/s; f64 bound = %d instructions per pair at 32.9 T/s (65.8 TFLOP/s of v_fma_f64, FMA = 2)
# host time: wall time of the call (a) itself, until it returns
""" % (REPS, WARMUP, TAPS, TAPS, N_JOBS, N_JOBS, N_JOBS, F64_OPS_PER_PAIR)


def setup(D):
    """the three routes as calls, and what to release afterwards"""
    x = ratelib.cutouts(fsea, D, JOB_BASE + D, N_SAMPLES, TAPS, N_JOBS)
    m = fsea.Measure()
    mjobs = (fsea.MeasureJob * N_JOBS)(*[fsea.MeasureJob(j.out_first + i % 2, JOB_BASE // D) for i, j in enumerate(x.table)])
    singles = [(fsea.MeasureJob * 1)(j) for j in mjobs]
    d_sums = fsea.DeviceBuffer(80 * N_JOBS)

    def a():
        m.run_device(x.d_pairs.ptr.value, x.total, mjobs, d_sums.ptr.value, offset=x.offset, lag=1)

    def c_route():
        for k, one in enumerate(singles):
            m.run_device(x.d_pairs.ptr.value, x.total, one, d_sums.ptr.value + 80 * k, offset=x.offset, lag=1)

    x.extract()
    return a, x.extract, c_route, (x.ex, m), (x.d_in, x.d_pairs, d_sums)


def measure(D):
    a, b, c_route, objects, buffers = setup(D)
    n_pairs = JOB_BASE // D
    (tb, tb_min), (ta, ta_min), (tc, tc_min) = (ratelib.median_min(ratelib.per_call(fn, WARMUP, REPS)) for fn in (b, a, c_route))
    # what the host spends inside the call (a) before it returns: checks, the table of 256 jobs, three launches
    sync = fsea.Plan(128)
    host = ratelib.host_time(a, sync.synchronize, REPS)
    sync.close()
    pairs = N_JOBS * n_pairs
    traffic, f64 = 8.0 * pairs / HBM_BPS, F64_OPS_PER_PAIR * pairs / F64_OPS_PER_S
    print("D=%-2d %d pairs in %d jobs   (a) measure %8.1f us (%8.1f)   (b) the extract call %8.1f us (%8.1f)   (c) %d one-job calls %9.1f us (%9.1f)"
          "   traffic bound %5.2f us   f64 bound %5.2f us   (a)/(b) %.3f   (c)/(a) %.1f   host time of (a) %.1f us"
          % (D, pairs, N_JOBS, ta * 1e6, ta_min * 1e6, tb * 1e6, tb_min * 1e6, N_JOBS, tc * 1e6, tc_min * 1e6, traffic * 1e6, f64 * 1e6,
             ta / tb, tc / ta, float(np.median(host)) * 1e6))
    ratelib.release(objects, buffers)


def launches():
    """what the trace sees: TRACE_CALLS calls of (a) at TRACE_D"""
    a, b, c_route, objects, buffers = setup(TRACE_D)
    ratelib.traced_calls(fsea, a, TRACE_CALLS)
    ratelib.release(objects, buffers)


def trace():
    times = ratelib.call_kernel_times(__file__, KERNELS, "fsea_measure_", TRACE_CALLS)
    print("kernel trace, D=%d, %d calls of (a): " % (TRACE_D, TRACE_CALLS) +
          "   ".join("%s %.1f us" % (k, t * 1e6) for k, t in zip(KERNELS, times)))


def main():
    if sys.argv[1:] == ["launches"]:         # the traced child of `trace`, not a part of its own
        return launches()
    parts = {"measure %d" % D: STEP_LIMIT_S for D in DECIMATIONS}
    parts["trace"] = STEP_LIMIT_S
    part = ratelib.run_parts(__file__, parts, sys.argv[1:], to=os.path.join(ROOT, "profiles", "measure_rate.txt"), header=HEADER + "\n")
    if part == "trace":
        trace()
    elif part:
        measure(int(part.split()[1]))


if __name__ == "__main__":
    main()
