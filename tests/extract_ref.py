"""A numpy restatement of fsea_extract_jobs and fsea_extract_layout, written from the contract in include/fsea.h, not from
the C, the reference of one job's pairs (tests/shift_ref.py's exact phase on the job's slice), and the recording of the
end-to-end tests (three tone bursts in noise) with the check they make of a cut-out."""
import numpy as np

from tests import shift_ref

JOB = np.dtype([("first", "<u8"), ("n_samples", "<u8"), ("sample_offset", "<u8"), ("cycles_per_sample", "<f8"),
                ("phase0_cycles", "<f8"), ("out_first", "<u8")])      # fsea_extract_job


def cutout_reference(iq, job, taps, D, flip):
    """The pairs of one job in f64: a job is a freshly reset zoom on its own samples (include/fsea.h), so this is
    shift_ref.zoom_reference on iq[2 first : 2 (first + n)] with the job's cycles_per_sample and phase0_cycles, its
    sample_offset as the stream position of sample 0 and a zero tail in front -- the phase exact, nothing of how the kernel
    groups or aligns its loads.  `job` is an fsea.ExtractJob or a JOB record; out_first is not looked at.  n_samples // D
    pairs; an empty job gives an empty array."""
    first, n, offset, cps, phase0 = (job[k] if isinstance(job, np.void) else getattr(job, k)
                                     for k in ("first", "n_samples", "sample_offset", "cycles_per_sample", "phase0_cycles"))
    first, n = int(first), int(n)
    if n == 0:
        return np.zeros(0, dtype=np.complex128)
    part = np.asarray(iq, dtype=np.uint8)[2 * first:2 * (first + n)]
    assert part.size == 2 * n, (first, n, "the job leaves the recording")
    return shift_ref.zoom_reference(part, flip, float(cps), float(phase0), taps, D, offset=int(offset))[0]


def lead(n_taps, decimation):
    """ceil((L - 1) / D) * D"""
    return -(-(n_taps - 1) // decimation) * decimation


def jobs(events, width, hop, n_samples, n_taps, decimation, max_fill=0.8):
    """(jobs as an array of JOB, fits as uint8): one job per event, in order."""
    out = np.zeros(len(events), dtype=JOB)
    fits = np.zeros(len(events), dtype=np.uint8)
    ld = lead(n_taps, decimation)
    for i, e in enumerate(events):
        row_first, row_last, col_first, col_last = (int(e[k]) for k in ("row_first", "row_last", "col_first", "col_last"))
        begin = row_first * hop
        first = begin - min(begin, ld)
        end = min(n_samples, row_last * hop + width)
        fits[i] = 1 if (col_last - col_first + 1) * decimation <= np.float64(max_fill) * np.float64(width) else 0
        out[i]["first"] = out[i]["sample_offset"] = first
        out[i]["n_samples"] = end - first if fits[i] and end > first else 0
        # the negated integer over the integer 2 N in one double division
        out[i]["cycles_per_sample"] = np.float64(-(col_first + col_last - 2 * (width // 2))) / np.float64(2 * width)
    return out, fits


def layout(n_samples, decimation):
    """(out_first per job, total pairs) for jobs of these lengths: each at the next even pair index, in order."""
    at, firsts = 0, []
    for n in n_samples:
        at = (at + 1) & ~1
        firsts.append(at)
        at += int(n) // decimation
    return firsts, at


# The recording of the end-to-end tests: N = H = 1024, 256 rows of int8 IQ (the tools' --flip), noise of sigma 20 with three
# tone bursts of amplitude 40 on whole frames at whole bins, so each burst is one column of its rows.  The bins are at
# least 100 from the centre: after the shift to a burst's centre the 0.5 of the offset-binary samples stands 100 bins or
# more away, 0.098 cycles per sample, far outside the low-pass of a decimation by 16 (half amplitude at 0.025).
N, ROWS, D, TAPS = 1024, 256, 16, 97
BURSTS = ((20, 60, 200), (100, 132, -300), (180, 250, 120))    # first row, the row behind the last, the bin from the centre
DETECTOR = (2, 16, 40, 0)                                     # guard, train, offset, CA
MIN_ROWS = 8                                                  # no run of noise detections stands for eight rows


def recording():
    rng = np.random.default_rng(77)
    x = rng.normal(0.0, 20.0, 2 * N * ROWS)
    for f0, f1, k in BURSTS:
        t = np.arange(f0 * N, f1 * N)
        tone = 40.0 * np.exp(2j * np.pi * (k / N) * t)
        x[2 * t] += tone.real
        x[2 * t + 1] += tone.imag
    return np.clip(np.rint(x), -128, 127).astype(np.int8).view(np.uint8)


def ideal_events():
    """the boxes of the injection as EVENTS_EVENT-like records"""
    ev = np.zeros(len(BURSTS), dtype=[("row_first", "<u4"), ("row_last", "<u4"), ("col_first", "<u4"), ("col_last", "<u4")])
    for i, (f0, f1, k) in enumerate(BURSTS):
        ev[i] = (f0, f1 - 1, N // 2 + k, N // 2 + k)
    return ev


def peak_bin_inside_the_burst(cutout, job_first, burst, rest=0.0):
    """The largest bin (as a signed bin number) of the FFT over the outputs of a cut-out (run-in dropped already) that lie
    inside the burst: output i of the job stands at sample job_first + i D.  `rest` is taken off every output first: the
    shifter puts its samples back round 0.5 + 0.5j after the rotation (fsea_fir_u8_shifted_*: rot_sample), so a cut-out rests
    on (0.5 + 0.5j) sum(c) and bin 0 is its largest whatever the shift; with that taken off, the largest bin is the emission."""
    ld = lead(TAPS, D)
    pos = job_first + (np.arange(cutout.size) + ld // D) * D
    # the taps of an output reach TAPS - 1 samples back: inside the burst from its first sample + TAPS - 1 on
    inside = cutout[(pos >= burst[0] * N + TAPS - 1) & (pos < burst[1] * N)]
    assert inside.size >= 1024, inside.size
    spectrum = np.abs(np.fft.fft(inside - rest))
    k = int(np.argmax(spectrum))
    return k if k <= inside.size // 2 else k - inside.size


def residual_bin(event, burst, n_inside):
    """Where the emission stands in that FFT when the job's centre is the middle of the event's box: the tone at column
    N / 2 + k, the shift to (col_first + col_last) / 2, the difference in cycles per sample times D per output, times the
    n_inside outputs of the FFT.  0 for a box centred on the tone; a box half a column off gives n_inside D / (2 N)."""
    off = N // 2 + burst[2] - (int(event["col_first"]) + int(event["col_last"])) / 2
    return off * D * n_inside / N


def inside_count(job_first, n_out, burst):
    pos = job_first + np.arange(lead(TAPS, D) // D, n_out) * D
    return int(((pos >= burst[0] * N + TAPS - 1) & (pos < burst[1] * N)).sum())
