#!/usr/bin/env python3
"""What the zoom spectrum (fsea_zoom_*, kernel fsea_shift_decim_u8) costs and buys, on a resident 64 MiB recording
(2^25 samples), L = 97, N = 1024, D = 4, 16, 64.

kernel:  HIP-event time of the decimating kernel -- a zoom object whose plan has a hop longer than the call, so a run_device
         call is that launch and one 128-point frame of the plan (one workgroup) behind it -- median of REPS launches after
         WARMUP, against its algorithmic traffic of 2 + 8 / D bytes per input sample at 8 TB/s.  The rotation (some twenty
         VALU operations per input sample) and the L / D packed FMAs are on top: the fraction says how far the kernel is
         from the memory bound, not what bounds it (the `counters` part under rocprofv3 --pmc says that).
rows:    end-to-end time for the same rows two ways, in this process on this data, median of CALLS after WARMUP_CALLS --
           zoom:   fsea_zoom_run_device on the resident recording, rows downloaded;
           parent: the only route before this object -- fsea_fir_u8_shifted_device at full rate, the pairs to the host,
                   every D-th kept in a host loop (numpy), fsea_exec_f64_host.
         The rows of the two are compared bit for bit first.
counters D: four launches at one D and nothing else, for a counters run of its own (rocprofv3 --pmc ... -- python
         scripts/zoom_rate.py counters 16), summarised by scripts/pmc_summary.py.

Without an argument kernel and rows run, each as a child process under its own time limit; a part that fails ends the run.
Usage: python scripts/zoom_rate.py [kernel|rows|counters D] [--to FILE]   (--to: what the parts print goes there too)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frequensea_amd import fsea  # noqa: E402
import ratelib  # noqa: E402

N_SAMPLES = 1 << 25
TAPS, FFT = 97, 1024
DECIMATIONS = (4, 16, 64)
CPS = -1.25e6 / 10e6
WARMUP, REPS = 5, 40
WARMUP_CALLS, CALLS = 2, 7
HBM_BPS = 8e12
STEP_LIMIT_S = {"kernel": 180, "rows": 420}


def taps_for(D):
    return fsea.lowpass_taps(10e6, 10e6 / (2 * D), TAPS)


def lone_kernel_zoom(D):
    """A zoom whose call is the decimating launch and a single 128-point frame: the hop is longer than any call here."""
    zoom = fsea.Zoom(taps_for(D), D, 128, 1 << 30)
    assert zoom.out_rows(N_SAMPLES) == 1
    return zoom


def kernel():
    import torch
    d_in, d_row = fsea.DeviceBuffer(2 * N_SAMPLES).upload(ratelib.recording(N_SAMPLES)), fsea.DeviceBuffer(128 * 4)
    torch.cuda.init()
    print("n = %d samples resident, L = %d; the decimating kernel alone, median of %d launches after %d" % (N_SAMPLES, TAPS, REPS, WARMUP))
    for D in DECIMATIONS:
        zoom = lone_kernel_zoom(D)
        times = ratelib.per_call(lambda: zoom.run_device(d_in.ptr.value, N_SAMPLES, d_row.ptr.value, CPS, flip=True), WARMUP, REPS)
        t = float(np.median(times))
        bound = (2.0 + 8.0 / D) * N_SAMPLES / HBM_BPS
        print("D=%-2d fsea_shift_decim_u8 median %8.1f us (min %8.1f)   traffic bound %6.1f us   fraction %.3f   %.1f Gsamples/s"
              % (D, t * 1e6, min(times) * 1e6, bound * 1e6, bound / t, N_SAMPLES / t / 1e9))
        zoom.close()
    d_in.free()
    d_row.free()


def rows():
    iq = ratelib.recording(N_SAMPLES)
    d_in = fsea.DeviceBuffer(iq.nbytes).upload(iq)
    print("n = %d samples resident, L = %d, N = %d; the same rows two ways, median (min) wall time of %d calls after %d"
          % (N_SAMPLES, TAPS, FFT, CALLS, WARMUP_CALLS))
    for D in DECIMATIONS:
        c = taps_for(D)
        zoom, fir, plan = fsea.Zoom(c, D, FFT), fsea.Fir(c), fsea.Plan(FFT, FFT, fsea.MODE_MAG_F32)
        n_rows = zoom.out_rows(N_SAMPLES)
        d_rows, d_full = fsea.DeviceBuffer(n_rows * FFT * 4), fsea.DeviceBuffer(8 * N_SAMPLES)

        def new_path():
            zoom.reset()
            zoom.run_device(d_in.ptr.value, N_SAMPLES, d_rows.ptr.value, CPS, flip=True)
            return d_rows.download(np.float32, (n_rows, FFT))      # a blocking copy on the null stream: waits for the launch

        def parent_path():
            fir.reset()
            fir.run_shifted_device(d_in.ptr.value, N_SAMPLES, d_full.ptr.value, CPS, flip=True)
            full = d_full.download(np.complex64, N_SAMPLES)
            kept = np.ascontiguousarray(full[::D][:N_SAMPLES // D])      # the host subsampling loop
            return plan.exec_host_f64(kept.view(np.float32).astype(np.float64), n_rows)

        assert np.array_equal(new_path().view(np.uint32), parent_path().view(np.uint32)), "the two routes differ"
        (zt, zmin), (pt, pmin) = (ratelib.median_min(ratelib.wall(fn, WARMUP_CALLS, CALLS)) for fn in (new_path, parent_path))
        print("D=%-2d %5d rows   zoom %9.1f us (%9.1f)   parent route %11.1f us (%11.1f)   ratio %.1f"
              % (D, n_rows, zt * 1e6, zmin * 1e6, pt * 1e6, pmin * 1e6, pt / zt))
        for obj in (zoom, fir, plan):
            obj.close()
        d_rows.free()
        d_full.free()
    d_in.free()


def counters(D):
    d_in, d_row = fsea.DeviceBuffer(2 * N_SAMPLES).upload(ratelib.recording(N_SAMPLES)), fsea.DeviceBuffer(128 * 4)
    sync = fsea.Plan(128)
    zoom = lone_kernel_zoom(D)
    for _ in range(4):
        zoom.run_device(d_in.ptr.value, N_SAMPLES, d_row.ptr.value, CPS, flip=True)
    sync.synchronize()
    zoom.close()
    sync.close()
    d_in.free()
    d_row.free()


def main():
    if sys.argv[1:2] == ["counters"]:
        counters(int(sys.argv[2]))
        return
    part = ratelib.run_parts(__file__, STEP_LIMIT_S, sys.argv[1:])
    if part:
        {"kernel": kernel, "rows": rows}[part]()


if __name__ == "__main__":
    main()
