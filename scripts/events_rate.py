#!/usr/bin/env python3
"""What the spectrum events' device passes cost (fsea_events_runs_device, fsea_events_paint_device) on a resident mask: the
DB5 rows of 4096 frames of N = 8192 of the bench's synthetic input (Gaussian noise, sigma 20, and a tone of amplitude 40 at
fs / 8; 32 MiB of rows), produced once by the plan, and the mask fsea_cfar_add_device makes of them at (G, T) = (2, 16).

In one process, with HIP events, the median of REPS calls after WARMUP:
  (a) the plan's launch that produces the rows;
  (b) fsea_cfar_add_device at (2, 16) with a mask;
  (c) fsea_events_runs_device on that mask with those rows as levels, at a column gap of 0 and of 3 -- the whole call, which
      waits for its own count in the middle and for the records at the end, and the counting call alone (capacity 0);
  (d) fsea_events_paint_device of all the runs found.
(c) is set against (b) and (a), and against its own traffic bound at 8 TB/s: the mask read twice, the 16-byte level groups
that hold a hit, the records written (the row counts, 4 bytes per row three times over, are left out).  The same for an
all-ones mask, the worst case for the level loads: every group is loaded, and a row is one run.

The measurement is one part, `run`; without an argument it runs as a child process under its time limit, and what it prints
also goes to profiles/events_rate.txt (--to FILE: there instead).
Usage: python scripts/events_rate.py [run] [--to FILE]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N, FRAMES = 8192, 4096
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
STEP_LIMIT_S = 120      # the whole part took 6.6 s of wall time on an MI355X
RUN_BYTES = fsea.EVENTS_RUN.itemsize


def synth_batch(seed, n_bytes):
    """bench.py's input: int8 IQ, Gaussian sigma 20 plus a complex tone at +fs / 8 of amplitude 40."""
    rng = np.random.default_rng(seed)
    n = n_bytes // 2
    out = np.empty(2 * n, dtype=np.int8)
    chunk = 1 << 22
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        ph = 2 * np.pi * 0.125 * np.arange(s, e, dtype=np.float64)
        out[2 * s:2 * e:2] = np.clip(np.rint(rng.normal(0, 20, e - s) + 40 * np.cos(ph)), -128, 127)
        out[2 * s + 1:2 * e:2] = np.clip(np.rint(rng.normal(0, 20, e - s) + 40 * np.sin(ph)), -128, 127)
    return out.view(np.uint8)


def run():
    if fsea.device_count() < 1:
        raise SystemExit("events_rate.py needs a GPU")
    import torch

    def say(text):
        print(text, flush=True)

    def med_min(call):
        return ratelib.median_min(ratelib.per_call(call, WARMUP, REPS))

    torch.cuda.init()
    raw = synth_batch(3, 2 * N * FRAMES)
    d_in = fsea.DeviceBuffer(raw.nbytes).upload(raw)
    d_rows = fsea.DeviceBuffer(FRAMES * N)
    d_mask = fsea.DeviceBuffer(FRAMES * N)
    d_image = fsea.DeviceBuffer(FRAMES * N)
    plan = fsea.Plan(N, N, fsea.MODE_DB5_U8_DCFIX)
    plan.exec_device(d_in.ptr.value, FRAMES, d_rows.ptr.value, flip=True)
    plan.synchronize()
    cfar = fsea.Cfar(N)
    cfar.set(2, 16, 60, fsea.CFAR_CA)
    say("%d rows x %d columns of DB5 rows resident (the bench's synthetic input); median of %d calls after %d, HIP events"
        % (FRAMES, N, REPS, WARMUP))
    pt, pmin = med_min(lambda: plan.exec_device(d_in.ptr.value, FRAMES, d_rows.ptr.value, flip=True))
    say("(a) the plan's launch that produces the rows:           %8.1f us (min %8.1f)" % (pt * 1e6, pmin * 1e6))
    ct, cmin = med_min(lambda: cfar.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask.ptr.value))
    say("(b) fsea_cfar_add_device at (2, 16) with a mask:        %8.1f us (min %8.1f)" % (ct * 1e6, cmin * 1e6))

    ev = fsea.Events(N)

    def measure(label, gap):
        mask = d_mask.download(np.uint8, (FRAMES, N))
        groups = int((mask.reshape(FRAMES, N // 16, 16) != 0).any(axis=2).sum())
        chunks = int((mask.reshape(FRAMES, N // 1024, 1024) != 0).any(axis=2).sum())
        ev.set_gap(gap)
        found = ev.runs_device(d_mask.ptr.value, FRAMES, None, 0)
        d_runs = fsea.DeviceBuffer(max(found, 1) * RUN_BYTES)
        d_values = fsea.DeviceBuffer(max(found, 1)).upload(np.full(max(found, 1), 255, np.uint8))

        def call():
            ev.reset()
            ev.runs_device(d_mask.ptr.value, FRAMES, d_runs.ptr.value, found, d_levels_ptr=d_rows.ptr.value, type=fsea.CFAR_U8)

        def count():
            ev.reset()
            ev.runs_device(d_mask.ptr.value, FRAMES, None, 0)

        t, tmin = med_min(call)
        t1, t1min = med_min(count)
        p, p_min = med_min(lambda: ev.paint_device(d_runs.ptr.value, d_values.ptr.value, found, FRAMES, d_image.ptr.value))
        read, written = 2 * FRAMES * N + 16 * groups, found * RUN_BYTES
        bound = (read + written) / HBM_BPS
        say("%s, column gap %d: %d hits in %d level groups of 16 and %d of the %d chunks of 1024, %d runs"
            % (label, gap, int((mask != 0).sum()), groups, chunks, FRAMES * N // 1024, found))
        say("  (c) fsea_events_runs_device with levels:            %8.1f us (min %8.1f)   the counting call alone %8.1f us (min %8.1f)"
            % (t * 1e6, tmin * 1e6, t1 * 1e6, t1min * 1e6))
        say("      (c) / (b) %.2f   (c) / (a) %.2f   bound %6.1f us (%d bytes read, %d written at 8 TB/s)   share of the bound %.3f"
            % (t / ct, t / pt, bound * 1e6, read, written, bound / t))
        say("  (d) fsea_events_paint_device of the %d runs:   %8.1f us (min %8.1f)   bound %6.1f us (the image written twice)"
            % (found, p * 1e6, p_min * 1e6, (2 * FRAMES * N + found * (RUN_BYTES + 1)) / HBM_BPS * 1e6))
        d_runs.free()
        d_values.free()

    measure("the detector's mask", 0)
    measure("the detector's mask", 3)
    d_mask.upload(np.full(FRAMES * N, 255, np.uint8))
    measure("an all-ones mask", 0)
    for o in (ev, cfar, plan):
        o.close()
    for b in (d_in, d_rows, d_mask, d_image):
        b.free()


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:], to=os.path.join(ROOT, "profiles", "events_rate.txt")):
        run()


if __name__ == "__main__":
    main()
