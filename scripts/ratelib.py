"""What the scripts/*_rate.py share: four ways to time a call, the kernel-trace reader, the part runner, the seeded
recording, for the two detectors' scripts the resident rows and the traffic count, and for the cut-out stages' scripts
the resident cut-outs and the per-kernel times of a call.  A script keeps its constants, its header text, the bound it
computes and its print lines; how a number is taken, and what more than one script measures on, is here, once.

Timing, all in seconds, each returning the list of its samples (the caller reduces: np.median, min, best of):
  per_call   HIP events round every single call;
  per_round  HIP events round `reps` back-to-back calls, `rounds` times, each divided by `reps`;
  wall       the host clock round every single call, for calls that end in a device wait;
  host_time  the host clock round every single call that does not wait, on a stream made idle outside the clock.

torch is imported inside the functions: a script decides when torch's HIP runtime loads relative to libfsea_hip.so
(tests/test_gpu_object_lifetime.py says why the order matters), and importing this module must not decide it for them."""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time
import types

import numpy as np


def per_call(call, warmup, reps):
    """`reps` times of one call each: fresh events on the null stream round every call, the first `warmup` results dropped."""
    import torch
    times = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            times.append(e0.elapsed_time(e1) / 1e3)
    return times


def per_round(call, warmup, reps, rounds):
    """`rounds` per-call times: `warmup` calls and a device wait, then events round `reps` back-to-back calls per round."""
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / 1e3 / reps)
    return out


def wall(call, warmup, calls):
    """`calls` host-clock times of one call each, after `warmup` untimed ones.  The call must end in a device wait (a
    blocking copy, a synchronize, a host form that downloads its result): the clock stops when the call returns, and
    whatever the device still has to do by then is not in the figure."""
    for _ in range(warmup):
        call()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return times


def host_time(call, idle, calls):
    """`calls` host-clock times of what the host spends inside a call that does not wait, before it returns: idle() brings
    the call's stream to rest outside the clock, and once more behind the last call.  Not `wall`: that clock stops when a
    call that ends in a device wait returns, this one when a call that left its work queued on an idle stream does."""
    times = []
    for _ in range(calls):
        idle()
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    idle()
    return times


def median_min(times):
    return float(np.median(times)), min(times)


def kernel_trace(argv, prefix, per_case, n_cases, out_dir=None):
    """Run `argv` in a fresh child under `rocprofv3 --kernel-trace` (nothing else traced, no counters) and read the
    dispatches of the kernels whose name starts with `prefix` (or with one of a tuple of them; the first names the trace),
    in start order: `per_case` of them for each of `n_cases` cases.  Returns per case (the first kernel's name, [durations
    in seconds]).  out_dir: keep the trace there, not in a temporary directory."""
    if out_dir is None:
        with tempfile.TemporaryDirectory() as tmp:
            return kernel_trace(argv, prefix, per_case, n_cases, tmp)
    prefix = (prefix,) if isinstance(prefix, str) else tuple(prefix)
    cmd = ["rocprofv3", "--kernel-trace", "-d", out_dir, "-o", prefix[0], "--output-format", "csv", "--"] + list(argv)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    traces = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(traces) != 1:
        raise SystemExit("expected one kernel trace under %s, found %d" % (out_dir, len(traces)))
    with open(traces[0], newline="") as f:
        rows = [r for r in csv.DictReader(f) if r["Kernel_Name"].startswith(prefix)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != per_case * n_cases:
        raise SystemExit("expected %d dispatches of %s, found %d" % (per_case * n_cases, " / ".join(prefix), len(rows)))
    cases = []
    for i in range(n_cases):
        mine = rows[i * per_case:(i + 1) * per_case]
        cases.append((mine[0]["Kernel_Name"], [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e9 for r in mine]))
    return cases


def _option(argv, flag):
    """(the value after `flag` or None, argv without the two)."""
    if flag not in argv:
        return None, argv
    i = argv.index(flag)
    return argv[i + 1], argv[:i] + argv[i + 2:]


def run_parts(script, parts, argv, to=None, header=""):
    """The GPU work of a script in parts, each a child process under a time limit of its own.

    parts: {part name: limit in seconds}, in the order they run; a name may be several words ("measure 16").
    argv:  the script's arguments.  `--to FILE` says where the text goes (instead of `to`); everything else, `--out DIR`
           (where a part keeps its trace) included, is the parts' own and is passed on to them.

    With a part name in argv: returns that name, and the script runs the part itself, in this process.  Without one: runs
    every part as `timeout -k 10 LIMIT python script part argv...`, echoes what each prints, and stops at the first that
    fails, starting nothing after it; after the last, writes `header` and what the parts printed to `to` (if there is
    one) and returns None."""
    file, argv = _option(list(argv), "--to")
    for name in parts:
        words = name.split()
        if any(argv[i:i + len(words)] == words for i in range(len(argv))):
            return name
    text = header
    for name, limit in parts.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(script)] + name.split() + argv,
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            raise SystemExit("%s failed (exit status %d): stopping" % (name, r.returncode))
        text += r.stdout
    if file or to:
        with open(file or to, "w") as f:
            f.write(text)
    return None


def recording(n_samples, seed=1):
    """n_samples of 8-bit IQ, two bytes each, uniform random from a seeded generator."""
    return np.random.default_rng(seed).integers(0, 256, 2 * n_samples, dtype=np.uint8)


def db5_rows(fsea, n, frames):
    """What the detectors' scripts measure on: the DB5 rows of `frames` frames of size n of the seeded recording, produced
    by the plan and left on the device.  Returns (plan, input buffer, rows buffer); the caller closes and frees them.
    `fsea` is the caller's frequensea_amd.fsea: this module imports no library."""
    raw = recording(n * frames)
    d_in = fsea.DeviceBuffer(raw.nbytes).upload(raw)
    d_rows = fsea.DeviceBuffer(frames * n)
    plan = fsea.Plan(n, n, fsea.MODE_DB5_U8_DCFIX)
    plan.exec_device(d_in.ptr.value, frames, d_rows.ptr.value, flip=True)
    plan.synchronize()
    return plan, d_in, d_rows


def detector_traffic(n, frames, tile, halo):
    """(bytes read, bytes written) of one detector add with mask on `frames` u8 rows of n cells: per row, every tile of
    `tile` columns with `halo` cells more each side, clipped at the row's ends; the mask.  How a kernel rounds its halo is
    the caller's."""
    per_row = sum(min(n, c0 + tile + halo) - max(0, c0 - halo) for c0 in range(0, n, tile))
    return frames * per_row, frames * n


def cutout_jobs(fsea, n_jobs, n_job):
    """The cut-out scripts' jobs: job i takes n_job samples from first = 131072 i + 3 + i mod 5, centre (i - 128) / 1024."""
    return [fsea.ExtractJob(131072 * i + 3 + i % 5, n_job, 131072 * i + 3 + i % 5, (i - 128) / 1024.0, 0.0, 0) for i in range(n_jobs)]


def cutouts(fsea, D, n_job, n_samples, n_taps, n_jobs):
    """What the cut-out stages' scripts measure on: the seeded recording of n_samples uploaded (d_in), the taps (c) of the
    low-pass for D, the Extract (ex), cutout_jobs laid out (table, total), the pairs buffer (d_pairs), the pedestal the
    pairs rest on (offset) and the extract call as a closure (extract); the caller runs it, and releases ex, d_in and
    d_pairs.  torch's HIP runtime is initialised between the upload, which loads the library, and everything else."""
    import torch
    iq = recording(n_samples)
    d_in = fsea.DeviceBuffer(iq.nbytes).upload(iq)
    torch.cuda.init()
    c = fsea.lowpass_taps(10e6, 10e6 / (2 * D), n_taps)
    ex = fsea.Extract(c, D)
    table, total = ex.layout(cutout_jobs(fsea, n_jobs, n_job))
    d_pairs = fsea.DeviceBuffer(8 * total)
    offset = 0.5 * float(np.sum(c.astype(np.float32).astype(np.float64))) * (1 + 1j)

    def extract():
        ex.run_device(d_in.ptr.value, n_samples, table, d_pairs.ptr.value, total, flip=True)

    return types.SimpleNamespace(d_in=d_in, c=c, ex=ex, table=table, total=total, d_pairs=d_pairs, offset=offset, extract=extract)


def release(objects, buffers):
    for o in objects:
        o.close()
    for o in buffers:
        o.free()


def traced_calls(fsea, call, n):
    """The traced child of call_kernel_times: n calls, then the device at rest."""
    for _ in range(n):
        call()
    sync = fsea.Plan(128)
    sync.synchronize()
    sync.close()


def call_kernel_times(script, kernels, family, calls):
    """The median seconds of each of `kernels`, a call's dispatches in launch order (the first is the table's upload, the
    others start with `family`), over the `calls` calls that `script launches` makes behind the one extract call -- which
    uploads a table too: the first dispatch of all, left out."""
    argv = [sys.executable, os.path.abspath(script), "launches"]
    name, times = kernel_trace(argv, (kernels[0], family), 1 + len(kernels) * calls, 1)[0]
    assert name.startswith(kernels[0]), name
    return [float(np.median(times[1 + i::len(kernels)])) for i in range(len(kernels))]
