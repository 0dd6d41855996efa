#!/usr/bin/env python3
"""What the ordered-statistic CFAR detector's add costs (fsea_oscfar_add_device with a mask, kernel fsea_oscfar_u8) on
resident rows: the DB5 rows of 4096 frames of N = 8192 (32 MiB), produced once by the plan and left on the device.

For (G, T, R) = (2, 16, 24) and (64, 256, 384): the HIP-event time of one add with mask, median of REPS calls after WARMUP.
Beside it, in the same process on the same rows:
  CA       the existing fsea_cfar_add_device (cell averaging) at the same (G, T): the prefix-sum kernel whose cost does not
           depend on T;
  traffic  the call's traffic bound at 8 TB/s -- the bytes read, every tile's segment with its halo of G + T cells (rounded up
           to whole 16-cell groups) each side clipped at the row's ends, plus the mask bytes written;
  compare  a compare bound: 2T compares per cell, VALU_PER_COMPARE vector instructions each (read off the shipped
           disassembly of fsea_oscfar_u8's count loop), at one wave-instruction per SIMD every four cycles of 2.4 GHz on
           256 CUs x 4 SIMDs; and the LDS bound of the same loop, LDS_BYTES_PER_COMPARE bytes per lane and compare at the
           LDS_BYTES_PER_CLK of the read instruction the loop uses.
The shares say how far the call is from each bound; the counters (`counters small|wide` under rocprofv3 --pmc, a run of its
own with no tracing beside it, summarised by scripts/pmc_summary.py) say which unit is busy.

The measurement is one part, `run`; without an argument it runs as a child process under its time limit, and what it prints
also goes to profiles/oscfar_rate.txt (--to FILE: there instead).
Usage: python scripts/oscfar_rate.py [run | counters small|wide] [--to FILE]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N, FRAMES = 8192, 4096
CASES = {"small": (2, 16, 24), "wide": (64, 256, 384)}
OFFSET = 60
WARMUP, REPS = 5, 20
HBM_BPS = 8e12
WAVE_INSTS_PER_S = 256 * 4 * 2.4e9 / 4      # every SIMD of every CU issuing one wave64 vector instruction per four cycles
VALU_PER_COMPARE = 1.5                      # a v_med3_i32 per compare and a v_add3_u32 for every two
LDS_BYTES_PER_COMPARE = 4.0                 # one level per lane: ds_read2_b32, two compares' levels
LDS_BYTES_PER_CLK = 128.0                   # per CU, ds_read_b32 / ds_read2_b32
STEP_LIMIT_S = 180


def traffic_bytes(guard, train):
    """(read, written) of one add with mask: per row, every tile's staged cells clipped at the row's ends; the mask."""
    return ratelib.detector_traffic(N, FRAMES, fsea.OSCFAR_TILE_COLUMNS, (guard + train + 15) // 16 * 16)


def resident_rows():
    plan, d_in, d_rows = ratelib.db5_rows(fsea, N, FRAMES)
    plan.close()
    d_in.free()
    return d_rows


def run():
    if fsea.device_count() < 1:
        raise SystemExit("oscfar_rate.py needs a GPU")
    import torch

    def say(text):
        print(text, flush=True)

    torch.cuda.init()
    d_rows = resident_rows()
    d_mask = fsea.DeviceBuffer(FRAMES * N)
    say("%d rows x %d columns of DB5 rows resident; fsea_oscfar_add_device with a mask, median of %d calls after %d"
        % (FRAMES, N, REPS, WARMUP))
    times = {}
    for name, (guard, train, rank) in CASES.items():
        ca = fsea.Cfar(N)
        ca.set(guard, train, OFFSET, fsea.CFAR_CA)
        ct, cmin = ratelib.median_min(ratelib.per_call(
            lambda: ca.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask.ptr.value), WARMUP, REPS))
        ca_hits = int(ca.hits().sum())
        ca.close()
        c = fsea.OsCfar(N)
        c.set(guard, train, OFFSET, rank)
        t, tmin = ratelib.median_min(ratelib.per_call(
            lambda: c.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask.ptr.value), WARMUP, REPS))
        detected, rows = int(c.hits().sum()), c.rows
        c.close()
        times[name] = t
        read, written = traffic_bytes(guard, train)
        traffic = (read + written) / HBM_BPS
        compares = FRAMES * N * 2 * train
        valu = compares / 64 * VALU_PER_COMPARE / WAVE_INSTS_PER_S
        lds = compares * LDS_BYTES_PER_COMPARE / (LDS_BYTES_PER_CLK * 256 * 2.4e9)
        say("(G, T, R) = (%2d, %3d, %3d): add %8.1f us (min %8.1f)   CA add on the same rows %8.1f us (min %8.1f)   OS / CA %.2f"
            % (guard, train, rank, t * 1e6, tmin * 1e6, ct * 1e6, cmin * 1e6, t / ct))
        say("    traffic bound %6.1f us (%d bytes read, %d written at 8 TB/s), share %.3f   compare bound %7.1f us "
            "(%.3g compares x %.1f VALU), share %.3f   LDS bound %7.1f us (%.0f B per compare at %.0f B/clk/CU), share %.3f"
            % (traffic * 1e6, read, written, traffic / t, valu * 1e6, compares, VALU_PER_COMPARE, valu / t, lds * 1e6,
               LDS_BYTES_PER_COMPARE, LDS_BYTES_PER_CLK, lds / t))
        say("    %.1f GB/s of rows   %.1f G compares/s   %d hits in %d rows (CA: %d hits)"
            % (FRAMES * N / t / 1e9, compares / t / 1e9, detected, rows, ca_hits))
    say("T = 16 -> 256 (16 x the compares): the add grows %.1f x" % (times["wide"] / times["small"]))
    for b in (d_rows, d_mask):
        b.free()


def counters(name):
    """Four adds at one setting and nothing else, for a counters run of its own."""
    if fsea.device_count() < 1:
        raise SystemExit("oscfar_rate.py needs a GPU")
    guard, train, rank = CASES[name]
    d_rows = resident_rows()
    d_mask = fsea.DeviceBuffer(FRAMES * N)
    c = fsea.OsCfar(N)
    c.set(guard, train, OFFSET, rank)
    for _ in range(4):
        c.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, d_mask.ptr.value)
    print("counters %s: %d hits in %d rows" % (name, int(c.hits().sum()), c.rows), flush=True)
    c.close()
    for b in (d_rows, d_mask):
        b.free()


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["counters"]:
        if argv[1:2] not in (["small"], ["wide"]):
            raise SystemExit("usage: oscfar_rate.py counters small|wide")
        counters(argv[1])
        return
    if ratelib.run_parts(__file__, {"run": STEP_LIMIT_S}, argv, to=os.path.join(ROOT, "profiles", "oscfar_rate.txt")):
        run()


if __name__ == "__main__":
    main()
