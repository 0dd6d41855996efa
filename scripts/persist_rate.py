#!/usr/bin/env python3
"""What the persistence spectrum's add costs (fsea_persist_add_device, kernel fsea_persist_u8), on a resident recording of
2^25 samples: the DB5 rows of N = 128, 1024 and 16384 (hop N, 2^25 bytes of rows each), produced once by the plan and left
on the device.

run:     HIP-event time of fsea_persist_add_device on those rows, median of REPS calls after WARMUP, as row bytes per
         second; beside it the comparator, the plan's own launch that produced the rows (fsea_exec_u8_device, code the
         persistence spectrum does not touch).
kernels: the add kernel alone, from the dispatch timestamps of a kernel trace: this part starts `rocprofv3 --kernel-trace`
         on the `launches` part (WARMUP + REPS adds per case, nothing else) and reads the trace; median per case beside the
         traffic bound at 8 TB/s -- n_rows * width bytes read, plus the flush: 4 bytes per non-zero counter of a
         workgroup's histogram, bounded above by all 256 * 64 of them for each of the (width / 64) * (n_rows / run)
         workgroups.  The fraction says how far the kernel is from the memory bound, not what bounds it.

Without an argument run and kernels run, each as a child process under its own time limit; a part that fails ends the run,
and what they print also goes to profiles/persist_rate.txt (--to FILE: there instead).
Usage: python scripts/persist_rate.py [run|kernels|launches] [--out DIR] [--to FILE]   (--out: keep the trace there)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N_SAMPLES = 1 << 25
SIZES = (128, 1024, 16384)
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
STEP_LIMIT_S = {"run": 240, "kernels": 300}
KERNEL = "fsea_persist_u8"


def resident_rows(d_in, n):
    """The DB5 rows of size n on the device: (plan, rows buffer, number of rows)."""
    plan = fsea.Plan(n, n, fsea.MODE_DB5_U8_DCFIX)
    frames = N_SAMPLES // n
    d_rows = fsea.DeviceBuffer(frames * n)
    plan.exec_device(d_in.ptr.value, frames, d_rows.ptr.value, flip=True)
    plan.synchronize()
    return plan, d_rows, frames


def run():
    import torch
    d_in = fsea.DeviceBuffer(2 * N_SAMPLES).upload(ratelib.recording(N_SAMPLES))
    torch.cuda.init()
    print("n = %d samples resident; fsea_persist_add_device on the DB5 rows (hop N), median of %d calls after %d"
          % (N_SAMPLES, REPS, WARMUP))
    for n in SIZES:
        plan, d_rows, frames = resident_rows(d_in, n)
        pt, pmin = ratelib.median_min(ratelib.per_call(lambda: plan.exec_device(d_in.ptr.value, frames, d_rows.ptr.value, flip=True),
                                                       WARMUP, REPS))
        p = fsea.Persist(n)
        t, tmin = ratelib.median_min(ratelib.per_call(lambda: p.add_device(d_rows.ptr.value, fsea.PERSIST_U8, frames, n), WARMUP, REPS))
        levels = int((p.counts().sum(axis=1) > 0).sum())
        print("N=%-5d rows %-6d  add %8.1f us (min %8.1f) %7.1f GB/s of rows   the plan's launch %8.1f us (min %8.1f)   add / plan %.2f   levels occupied %d"
              % (n, frames, t * 1e6, tmin * 1e6, frames * n / t / 1e9, pt * 1e6, pmin * 1e6, t / pt, levels))
        p.close()
        plan.close()
        d_rows.free()
    d_in.free()


def launches():
    d_in = fsea.DeviceBuffer(2 * N_SAMPLES).upload(ratelib.recording(N_SAMPLES))
    for n in SIZES:
        plan, d_rows, frames = resident_rows(d_in, n)
        p = fsea.Persist(n)
        for _ in range(WARMUP + REPS):
            p.add_device(d_rows.ptr.value, fsea.PERSIST_U8, frames, n)
        plan.synchronize()
        p.close()
        plan.close()
        d_rows.free()
    d_in.free()


def kernel_times(out_dir):
    cases = ratelib.kernel_trace([sys.executable, os.path.abspath(__file__), "launches"], KERNEL, WARMUP + REPS, len(SIZES), out_dir)
    print("n = %d samples resident; %s alone (dispatch timestamps of a kernel trace), median of %d launches after %d"
          % (N_SAMPLES, KERNEL, REPS, WARMUP))
    for n, (name, times) in zip(SIZES, cases):
        t, tmin = ratelib.median_min(times[WARMUP:])
        frames = N_SAMPLES // n
        groups = -(-n // 64) * -(-frames // fsea.PERSIST_RUN_ROWS)
        read = frames * n / HBM_BPS
        flush_max = groups * 256 * 64 * 4 / HBM_BPS
        print("N=%-5d %s median %8.1f us (min %8.1f)   %d workgroups   bound: rows %5.1f us, rows + every counter flushed %5.1f us   fraction %.3f .. %.3f   %.1f GB/s of rows"
              % (n, name, t * 1e6, tmin * 1e6, groups, read * 1e6, (read + flush_max) * 1e6, read / t,
                 (read + flush_max) / t, frames * n / t / 1e9))


def main():
    args = sys.argv[1:]
    if "launches" in args:
        launches()
        return
    part = ratelib.run_parts(__file__, STEP_LIMIT_S, args, to=os.path.join(ROOT, "profiles", "persist_rate.txt"))
    if part == "run":
        run()
    elif part == "kernels":
        kernel_times(args[args.index("--out") + 1] if "--out" in args else None)


if __name__ == "__main__":
    main()
