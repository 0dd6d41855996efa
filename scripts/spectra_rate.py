#!/usr/bin/env python3
"""What the averaged spectra of a table of cut-outs (fsea_spectra_*, kernels fsea_spectra_tiles_<n> and fsea_spectra_fold)
cost, on N_JOBS jobs of 2^16 resident f32 pairs each, n = 256, 1024 and 4096 at hop n / 2, Hann taper, kinds z and fourth.
HIP-event times in one process, median of REPS calls after WARMUP:

(a) one fsea_spectra_run_device of the table, the jobs at even and odd firsts in turn;
(b) the same spans as one fsea_plan run per job in mode complex (fsea_exec_u8_device at the same n and hop, Hann window, on
    2^16 8-bit samples a job): the route a caller has without the job table.  It reads 2 bytes a sample where (a) reads 8, it
    writes every frame's row of n complex values, which nothing averages and the caller throws away, and it costs a launch
    per job.

The roofline of (a): 8 bytes per pair read and 4 n bytes per job written, at 8 TB/s; a pair is read twice at hop n / 2 and
the second time from a cache, so the bytes that must move are the pairs once.

Without an argument every n runs as a child process under its own time limit and the lines go to
profiles/spectra_rate.txt (or the file named after --to); a part that fails ends the run.
Usage: python scripts/spectra_rate.py [--to FILE] | python scripts/spectra_rate.py measure N      (N = 256, 1024 or 4096)"""
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

SIZES = (256, 1024, 4096)
KINDS = ("z", "fourth")
N_JOBS, JOB_PAIRS = 256, 1 << 16
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
STEP_LIMIT_S = 240


def host_cpu():
    """the box's CPU as /proc/cpuinfo names it"""
    try:
        with open("/proc/cpuinfo") as f:
            return next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        return platform.processor() or platform.machine()


HEADER = """# scripts/spectra_rate.py on one MI355X: HIP-event times in one process, median (min) of %d calls after %d
# box: one MI355X (gfx950), host CPU %s; %s UTC
# %d jobs of 2^16 f32 pairs resident (seeded noise on a 0.5 + 0.5j pedestal), first_pair = 65538 i + i mod 2; hop n / 2, Hann taper
# (a) one fsea_spectra_run_device of the table
# (b) %d fsea_exec_u8_device calls, one per job, of a plan of n, hop n / 2, mode complex, Hann window, on 2^16 8-bit samples a job:
#     the rows of every frame written and thrown away, nothing averaged
# roofline of (a) = 8 bytes per pair read + 4 n bytes per job written, at 8 TB/s
""" % (REPS, WARMUP, host_cpu(), time.strftime("%Y-%m-%d %H:%M", time.gmtime()), N_JOBS, N_JOBS)


def measure(n):
    import torch
    rng = np.random.default_rng(1)
    total = N_JOBS * (JOB_PAIRS + 2)
    pairs = np.empty(total, np.complex64)
    pairs.real = rng.standard_normal(total, dtype=np.float32) + np.float32(0.5)
    pairs.imag = rng.standard_normal(total, dtype=np.float32) + np.float32(0.5)
    d_pairs = fsea.DeviceBuffer(pairs.nbytes).upload(pairs)
    iq = ratelib.recording(N_JOBS * JOB_PAIRS)
    d_iq = fsea.DeviceBuffer(iq.nbytes).upload(iq)
    torch.cuda.init()
    hop = n // 2
    w = fsea.window("hann", n)
    frames = (JOB_PAIRS - n) // hop + 1
    plan = fsea.Plan(n, hop, fsea.MODE_COMPLEX_F32)
    plan.set_window(w)
    d_rows = fsea.DeviceBuffer(frames * plan.row_bytes)

    def b():
        for i in range(N_JOBS):
            plan.exec_device(d_iq.ptr.value + 2 * JOB_PAIRS * i, frames, d_rows.ptr.value)

    tb, tb_min = ratelib.median_min(ratelib.per_call(b, WARMUP, REPS))
    sync = fsea.Plan(128)
    for kind in KINDS:
        sp = fsea.Spectra(n, hop, kind, w)
        assert sp.segments(JOB_PAIRS) == frames
        table, floats = sp.layout([fsea.SpectraJob((JOB_PAIRS + 2) * i + i % 2, JOB_PAIRS, 0) for i in range(N_JOBS)])
        d_power = fsea.DeviceBuffer(4 * floats)

        def a():
            sp.run_device(d_pairs.ptr.value, total, table, d_power.ptr.value, floats, offset=0.5 + 0.5j)

        ta, ta_min = ratelib.median_min(ratelib.per_call(a, WARMUP, REPS))
        host = ratelib.host_time(a, sync.synchronize, REPS)
        n_pairs = N_JOBS * JOB_PAIRS
        bound = (8.0 * n_pairs + 4.0 * n * N_JOBS) / HBM_BPS
        print("n=%-4d kind %-6s %d pairs in %d jobs, %d segments a job   (a) spectra %8.1f us (%8.1f)   %7.2f G pairs/s   roofline %6.2f us: %5.1f %% of 8 TB/s"
              "   (b) %d plan runs %9.1f us (%9.1f)   (b)/(a) %.1f   host time of (a) %.1f us"
              % (n, kind, n_pairs, N_JOBS, frames, ta * 1e6, ta_min * 1e6, n_pairs / ta / 1e9, bound * 1e6, 100.0 * bound / ta, N_JOBS,
                 tb * 1e6, tb_min * 1e6, tb / ta, float(np.median(host)) * 1e6))
        sp.close()
        d_power.free()
    for o in (plan, sync):
        o.close()
    for o in (d_pairs, d_iq, d_rows):
        o.free()


def main():
    parts = {"measure %d" % n: STEP_LIMIT_S for n in SIZES}
    part = ratelib.run_parts(__file__, parts, sys.argv[1:], to=os.path.join(ROOT, "profiles", "spectra_rate.txt"), header=HEADER + "\n")
    if part:
        measure(int(part.split()[1]))


if __name__ == "__main__":
    main()
