#!/usr/bin/env python3
"""What the polyphase filter bank (fsea_pfb_*, kernel fsea_pfb_frames_u8) costs, on a resident 64 MiB recording (2^25
samples), (M, P, q) = (128, 8, 1), (1024, 8, 1), (1024, 8, 2), (16384, 4, 1), MAG rows.

run:     HIP-event time of a whole fsea_pfb_run_device call (the frames kernel and the plan's launch on the frames behind
         it), median of REPS calls after WARMUP, as input samples per second; beside it the comparator, the same recording
         through a Hann-windowed fsea.Plan(M) (fsea_exec_u8_device, hop M / q): what the bank costs over a plain windowed row.
kernels: the frames kernel alone.  A call always runs the plan behind it, so its time is taken from the dispatch
         timestamps of a kernel trace: this part starts `rocprofv3 --kernel-trace` on the `launches` part (WARMUP + REPS
         calls per case, nothing else) and reads the trace; median per case, samples per second, and the fraction of 8 TB/s
         at the kernel's algorithmic traffic of 2 + 8 q bytes per input sample (2 read, a frame of M pairs written every
         M / q samples).  The fraction says how far the kernel is from the memory bound, not what bounds it.

Without an argument run and kernels run, each as a child process under its own time limit; a part that fails ends the run.
Usage: python scripts/pfb_rate.py [run|kernels|launches] [--out DIR] [--to FILE]   (--out: keep the trace there; --to: what
the parts print goes there too -- profiles/pfb_rate.txt is the output of a run without a part)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N_SAMPLES = 1 << 25
CASES = ((128, 8, 1), (1024, 8, 1), (1024, 8, 2), (16384, 4, 1))
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
STEP_LIMIT_S = {"run": 240, "kernels": 300}
KERNEL = "fsea_pfb_frames_u8"


def run():
    import torch
    d_in = fsea.DeviceBuffer(2 * N_SAMPLES).upload(ratelib.recording(N_SAMPLES))
    torch.cuda.init()
    print("n = %d samples resident; a whole call (frames kernel + plan), median of %d calls after %d, MAG rows"
          % (N_SAMPLES, REPS, WARMUP))
    for M, P, q in CASES:
        D = M // q
        pfb = fsea.Pfb(fsea.pfb_prototype(M, P), M, q, fsea.MODE_MAG_F32)
        F = pfb.out_frames(N_SAMPLES)
        d_rows = fsea.DeviceBuffer(F * M * 4)
        t, tmin = ratelib.median_min(ratelib.per_call(lambda: pfb.run_device(d_in.ptr.value, N_SAMPLES, d_rows.ptr.value, flip=True),
                                                     WARMUP, REPS))
        pfb.close()
        plan = fsea.Plan(M, D, fsea.MODE_MAG_F32)
        plan.set_window("hann")
        nf = (N_SAMPLES - M) // D + 1
        d_plain = fsea.DeviceBuffer(nf * M * 4)
        pt, pmin = ratelib.median_min(ratelib.per_call(lambda: plan.exec_device(d_in.ptr.value, nf, d_plain.ptr.value, flip=True),
                                                       WARMUP, REPS))
        plan.close()
        print("M=%-5d P=%-2d q=%d  bank %9.1f us (min %9.1f) %6.2f Gsamples/s   Hann-windowed plan %9.1f us (min %9.1f) %6.2f Gsamples/s   ratio %.2f"
              % (M, P, q, t * 1e6, tmin * 1e6, N_SAMPLES / t / 1e9, pt * 1e6, pmin * 1e6, N_SAMPLES / pt / 1e9, t / pt))
        d_rows.free()
        d_plain.free()
    d_in.free()


def launches():
    d_in = fsea.DeviceBuffer(2 * N_SAMPLES).upload(ratelib.recording(N_SAMPLES))
    sync = fsea.Plan(128)
    for M, P, q in CASES:
        pfb = fsea.Pfb(fsea.pfb_prototype(M, P), M, q, fsea.MODE_MAG_F32)
        d_rows = fsea.DeviceBuffer(pfb.out_frames(N_SAMPLES) * M * 4)
        for _ in range(WARMUP + REPS):
            pfb.run_device(d_in.ptr.value, N_SAMPLES, d_rows.ptr.value, flip=True)
        sync.synchronize()
        pfb.close()
        d_rows.free()
    sync.close()
    d_in.free()


def kernel_times(out_dir):
    cases = ratelib.kernel_trace([sys.executable, os.path.abspath(__file__), "launches"], KERNEL, WARMUP + REPS, len(CASES), out_dir)
    print("n = %d samples resident; %s alone (dispatch timestamps of a kernel trace), median of %d launches after %d"
          % (N_SAMPLES, KERNEL, REPS, WARMUP))
    for (M, P, q), (name, times) in zip(CASES, cases):
        t, tmin = ratelib.median_min(times[WARMUP:])
        bound = (2.0 + 8.0 * q) * N_SAMPLES / HBM_BPS
        print("M=%-5d P=%-2d q=%d  %s median %8.1f us (min %8.1f)   traffic bound %6.1f us   fraction %.3f   %.2f Gsamples/s"
              % (M, P, q, name, t * 1e6, tmin * 1e6, bound * 1e6, bound / t, N_SAMPLES / t / 1e9))


def main():
    args = sys.argv[1:]
    if "launches" in args:
        launches()
        return
    part = ratelib.run_parts(__file__, STEP_LIMIT_S, args)
    if part == "run":
        run()
    elif part == "kernels":
        kernel_times(args[args.index("--out") + 1] if "--out" in args else None)


if __name__ == "__main__":
    main()
