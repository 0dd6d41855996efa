#!/usr/bin/env python3
"""What a table of cut-outs in one launch (fsea_extract_*, kernel fsea_extract_u8) costs against the zoom it shares its
arithmetic with, on a resident recording of 2^25 samples, L = 97, D = 4, 16, 64.  HIP-event times in one process, median of
REPS calls after WARMUP:

(a) one fsea_extract_run_device of 256 jobs of 65536 + D - 1 samples each, spread over the recording at firsts that are no
    multiples of 8, every job with its own centre;
(b) one fsea_zoom_run_device over the same total number of samples (a zoom whose plan yields a single 128-point frame, as
    scripts/zoom_rate.py times the decimating kernel);
(c) 256 fsea_zoom_run_device calls of one job's length each: the route before this object, without the resets it would
    also need.

(a) / (b) is what the ragged last tile of every job, the table look-up and the misaligned ends cost; (c) / (a) is what the
one launch buys.  The traffic bound is 2 + 8 / D bytes per input sample at 8 TB/s, as in profiles/zoom_rate.txt.

Without an argument every D runs as a child process under its own time limit and the lines go to profiles/extract_rate.txt
(or the file named after --to); a part that fails ends the run.
Usage: python scripts/extract_rate.py [--to FILE] | python scripts/extract_rate.py measure D      (D = 4, 16 or 64)"""
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
STEP_LIMIT_S = 240

HEADER = """# scripts/extract_rate.py on one MI355X: HIP-event times in one process, median (min) of %d calls after %d
# recording: 2^25 samples resident, L = %d, taps = lowpass(10e6, 10e6 / (2 D), %d)
# (a) one fsea_extract_run_device: %d jobs of 65536 + D - 1 samples, first = 131072 i + 3 + i mod 5, a centre per job
# (b) one fsea_zoom_run_device over the same number of samples (its plan yields one 128-point frame)
# (c) %d fsea_zoom_run_device calls of one job's length each, no resets
# traffic bound = (2 + 8 / D) bytes per input sample at 8 TB/s; host time: wall time of the call (a) itself, until it returns
""" % (REPS, WARMUP, TAPS, TAPS, N_JOBS, N_JOBS)


def measure(D):
    n_job = JOB_BASE + D - 1
    total_samples = N_JOBS * n_job
    x = ratelib.cutouts(fsea, D, n_job, N_SAMPLES, TAPS, N_JOBS)
    a, d_in = x.extract, x.d_in
    zoom = fsea.Zoom(x.c, D, 128, 1 << 30)
    assert zoom.out_rows(total_samples) == 1 and zoom.out_rows(n_job) == 1
    d_row = fsea.DeviceBuffer(128 * 4)

    def b():
        zoom.run_device(d_in.ptr.value, total_samples, d_row.ptr.value, -0.125, flip=True)

    def c_route():
        for j in x.table:
            zoom.run_device(d_in.ptr.value + 2 * (j.first & ~7), n_job, d_row.ptr.value, j.cycles_per_sample,
                            sample_offset=j.sample_offset, flip=True)

    (ta, ta_min), (tb, tb_min), (tc, tc_min) = (ratelib.median_min(ratelib.per_call(fn, WARMUP, REPS)) for fn in (a, b, c_route))
    # what the host spends inside the call before it returns: checks, 256 records with eight phasors each, two launches
    sync = fsea.Plan(128)
    host = ratelib.host_time(a, sync.synchronize, REPS)
    sync.close()
    bound = (2.0 + 8.0 / D) * total_samples / HBM_BPS
    print("D=%-2d %d samples in %d jobs   (a) extract %8.1f us (%8.1f)   (b) one zoom call %8.1f us (%8.1f)   (c) %d zoom calls %9.1f us (%9.1f)"
          "   traffic bound %5.1f us   (a)/(b) %.3f   (c)/(a) %.1f   host time of (a) %.1f us"
          % (D, total_samples, N_JOBS, ta * 1e6, ta_min * 1e6, tb * 1e6, tb_min * 1e6, N_JOBS, tc * 1e6, tc_min * 1e6, bound * 1e6, ta / tb,
             tc / ta, float(np.median(host)) * 1e6))
    ratelib.release((x.ex, zoom), (d_in, x.d_pairs, d_row))


def main():
    part = ratelib.run_parts(__file__, {"measure %d" % D: STEP_LIMIT_S for D in DECIMATIONS}, sys.argv[1:],
                             to=os.path.join(ROOT, "profiles", "extract_rate.txt"), header=HEADER + "\n")
    if part:
        measure(int(part.split()[1]))


if __name__ == "__main__":
    main()
