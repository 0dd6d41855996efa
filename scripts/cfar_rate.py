#!/usr/bin/env python3
"""What the CFAR detector's add costs (fsea_cfar_add_device with a mask, kernel fsea_cfar_u8) on resident rows: the DB5 rows
of 4096 frames of N = 8192 (32 MiB), produced once by the plan and left on the device.

For (G, T) = (2, 16) and (64, 256): the HIP-event time of one add with mask, median of REPS calls after WARMUP, as a share of
the call's traffic bound at 8 TB/s -- the bytes read, every tile's segment with its halo of G + T cells each side clipped at
the row's ends, plus the mask bytes written; the share says how far the call is from the memory bound, not what bounds it.
Beside it the ratio to the plan's own launch that produced those rows (fsea_exec_u8_device, code the detector does not
touch), measured in the same process.

The measurement is one part, `run`; without an argument it runs as a child process under its time limit, and what it prints
also goes to profiles/cfar_rate.txt (--to FILE: there instead).
Usage: python scripts/cfar_rate.py [run] [--to FILE]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N, FRAMES = 8192, 4096
CASES = ((2, 16), (64, 256))
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
STEP_LIMIT_S = 120      # the whole part took 13.0 s of wall time on an MI355X


def traffic_bytes(guard, train):
    """(read, written) of one add with mask: per row, every tile's segment clipped at the row's ends; the mask."""
    return ratelib.detector_traffic(N, FRAMES, fsea.CFAR_TILE_COLUMNS, guard + train)


def run():
    if fsea.device_count() < 1:
        raise SystemExit("cfar_rate.py needs a GPU")
    import torch

    def say(text):
        print(text, flush=True)

    torch.cuda.init()
    plan, d_in, d_rows = ratelib.db5_rows(fsea, N, FRAMES)
    d_mask = fsea.DeviceBuffer(FRAMES * N)
    say("%d rows x %d columns of DB5 rows resident; fsea_cfar_add_device with a mask, median of %d calls after %d"
        % (FRAMES, N, REPS, WARMUP))
    pt, pmin = ratelib.median_min(ratelib.per_call(lambda: plan.exec_device(d_in.ptr.value, FRAMES, d_rows.ptr.value, flip=True),
                                                   WARMUP, REPS))
    say("the plan's launch that produces the rows: %8.1f us (min %8.1f)" % (pt * 1e6, pmin * 1e6))
    for guard, train in CASES:
        c = fsea.Cfar(N)
        c.set(guard, train, 60, fsea.CFAR_CA)
        t, tmin = ratelib.median_min(ratelib.per_call(
            lambda: c.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask.ptr.value), WARMUP, REPS))
        detected = int(c.hits().sum())
        rows = c.rows
        c.close()
        read, written = traffic_bytes(guard, train)
        bound = (read + written) / HBM_BPS
        say("(G, T) = (%2d, %3d): add %8.1f us (min %8.1f)   bound %6.1f us (%d bytes read, %d written at 8 TB/s)   "
            "share of the bound %.3f   add / plan %.2f   %.1f GB/s of rows   %d hits in %d rows"
            % (guard, train, t * 1e6, tmin * 1e6, bound * 1e6, read, written, bound / t, t / pt, FRAMES * N / t / 1e9, detected, rows))
    plan.close()
    for b in (d_in, d_rows, d_mask):
        b.free()


def main():
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, sys.argv[1:], to=os.path.join(ROOT, "profiles", "cfar_rate.txt")):
        run()


if __name__ == "__main__":
    main()
