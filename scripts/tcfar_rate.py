#!/usr/bin/env python3
"""What the time-axis CFAR detector's add costs (fsea_tcfar_add_device with a mask, kernel fsea_tcfar_u8) on resident rows:
the DB5 rows of 4096 frames of N = 8192 (32 MiB), produced once by the plan and left on the device.

For (G, T) = (2, 16) and (64, 256): the HIP-event time of one add with mask, median of REPS calls after WARMUP.  Beside it,
in the same process on the same rows:
  CA       the existing fsea_cfar_add_device (cell averaging across frequency) at the same (G, T);
  traffic  the call's traffic bound at 8 TB/s -- the rows read once, the prologue rows of every workgroup (the T rows of each
           window of its run's first row, clipped to the rows of the call), and the mask bytes written.  The four lagging
           streams of a run re-read rows the leading stream touched at most 2 (G + T) + 1 rows earlier; the bound takes
           them to come from a cache;
  loads    what the kernel asks of the caches: five row reads per decided row and tile beside the prologue's.
The shares say how far the call is from the bound; the counters (`counters small|wide` under rocprofv3 --pmc, a run of its
own with no tracing beside it, summarised by scripts/pmc_summary.py) say which unit is busy.

The measurement is one part, `run`; without an argument it runs as a child process under its time limit, and what it prints
also goes to profiles/tcfar_rate.txt (--to FILE: there instead).
Usage: python scripts/tcfar_rate.py [run | counters small|wide] [--to FILE]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N, FRAMES = 8192, 4096
CASES = {"small": (2, 16), "wide": (64, 256)}
OFFSET = 60
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
STEP_LIMIT_S = 180


def prologue_rows(guard, train, run):
    """The rows the workgroups of one tile read to build the window sums of their runs' first rows."""
    total = 0
    for r in range(0, FRAMES, run):
        total += max(0, min(r - guard - 1, FRAMES - 1) - max(r - guard - train, 0) + 1)
        total += max(0, min(r + guard + train, FRAMES - 1) - max(r + guard + 1, 0) + 1)
    return total


def traffic_bytes(guard, train, run):
    """(read, written, loaded) of one add with mask: the rows once and every workgroup's prologue rows; the mask; and the
    bytes of all row reads the kernel issues."""
    prologue = prologue_rows(guard, train, run) * N
    return FRAMES * N + prologue, FRAMES * N, 5 * FRAMES * N + prologue


def resident_rows():
    plan, d_in, d_rows = ratelib.db5_rows(fsea, N, FRAMES)
    plan.close()
    d_in.free()
    return d_rows


def run():
    if fsea.device_count() < 1:
        raise SystemExit("tcfar_rate.py needs a GPU")
    import torch

    def say(text):
        print(text, flush=True)

    torch.cuda.init()
    d_rows = resident_rows()
    d_mask = fsea.DeviceBuffer(FRAMES * N)
    say("%d rows x %d columns of DB5 rows resident; fsea_tcfar_add_device with a mask, median of %d calls after %d"
        % (FRAMES, N, REPS, WARMUP))
    times = {}
    for name, (guard, train) in CASES.items():
        ca = fsea.Cfar(N)
        ca.set(guard, train, OFFSET, fsea.CFAR_CA)
        ct, cmin = ratelib.median_min(ratelib.per_call(
            lambda: ca.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask.ptr.value), WARMUP, REPS))
        ca_hits = int(ca.hits().sum())
        ca.close()
        c = fsea.Tcfar(N)
        c.set(guard, train, OFFSET, fsea.CFAR_CA)
        run_rows = c.run_rows
        t, tmin = ratelib.median_min(ratelib.per_call(
            lambda: c.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask_ptr=d_mask.ptr.value), WARMUP, REPS))
        detected, rows = int(c.hits().sum()), c.rows
        c.close()
        times[name] = t
        read, written, loaded = traffic_bytes(guard, train, run_rows)
        traffic = (read + written) / HBM_BPS
        workgroups = -(-FRAMES // run_rows) * -(-N // fsea.TCFAR_TILE_COLUMNS)
        say("(G, T) = (%2d, %3d): add %8.1f us (min %8.1f)   CA add across frequency on the same rows %8.1f us (min %8.1f)   time / CA %.2f"
            % (guard, train, t * 1e6, tmin * 1e6, ct * 1e6, cmin * 1e6, t / ct))
        say("    traffic bound %6.1f us (%d bytes read, %d written at 8 TB/s), share %.3f   %d workgroups of one wave, runs of %d rows"
            % (traffic * 1e6, read, written, traffic / t, workgroups, run_rows))
        say("    %.1f GB/s of rows   %.2f TB/s of row reads asked of the caches (%d bytes)   %d hits in %d rows (CA: %d hits)"
            % (FRAMES * N / t / 1e9, loaded / t / 1e12, loaded, detected, rows, ca_hits))
    say("T = 16 -> 256 (16 x the prologue): the add grows %.2f x" % (times["wide"] / times["small"]))
    for b in (d_rows, d_mask):
        b.free()


def counters(name):
    """Four adds at one setting and nothing else, for a counters run of its own."""
    if fsea.device_count() < 1:
        raise SystemExit("tcfar_rate.py needs a GPU")
    guard, train = CASES[name]
    d_rows = resident_rows()
    d_mask = fsea.DeviceBuffer(FRAMES * N)
    c = fsea.Tcfar(N)
    c.set(guard, train, OFFSET, fsea.CFAR_CA)
    for _ in range(4):
        c.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask_ptr=d_mask.ptr.value)
    print("counters %s: %d hits in %d rows" % (name, int(c.hits().sum()), c.rows), flush=True)
    c.close()
    for b in (d_rows, d_mask):
        b.free()


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["counters"]:
        if argv[1:2] not in (["small"], ["wide"]):
            raise SystemExit("usage: tcfar_rate.py counters small|wide")
        counters(argv[1])
        return
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, argv, to=os.path.join(ROOT, "profiles", "tcfar_rate.txt")):
        run()


if __name__ == "__main__":
    main()
