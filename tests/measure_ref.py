"""A numpy restatement of fsea_measure_*, written from the contract in include/fsea.h, not from the kernels: the terms of a
job in f64 with the header's roundings (numpy rounds every product and every sum on its own), fold_W as vectorised adds
over the steps and the xor stages, a job's record as the 80 bytes of fsea_measure_sums; fsea_measure_jobs and
fsea_measure_finish as their formulas."""
import numpy as np

TILE = 4096
SUMS = np.dtype([("s_re", "<f8"), ("s_im", "<f8"), ("p", "<f8"), ("q", "<f8"), ("r_re", "<f8"), ("r_im", "<f8"), ("peak", "<f8"),
                 ("peak_index", "<u8"), ("n_pairs", "<u8"), ("n_lagged", "<u8")])        # fsea_measure_sums
JOB = np.dtype([("first_pair", "<u8"), ("n_pairs", "<u8")])                            # fsea_measure_job
NAMES = ("s_re", "s_im", "p", "q", "r_re", "r_im")


def terms(pairs, offset=0j, lag=1):
    """The six term arrays (a, b, P, Q, Rre, Rim) of a job's pairs, one f64 each per pair; the R terms of i < lag are +0.0."""
    z = np.ascontiguousarray(pairs, dtype=np.complex64).ravel()
    offset = complex(offset)
    a = z.real.astype(np.float64) - np.float64(offset.real)
    b = z.imag.astype(np.float64) - np.float64(offset.imag)
    p = a * a + b * b
    q = p * p
    r_re, r_im = np.zeros(z.size), np.zeros(z.size)
    if lag < z.size:
        ai, bi, aj, bj = a[lag:], b[lag:], a[:z.size - lag], b[:z.size - lag]
        r_re[lag:] = ai * aj + bi * bj
        r_im[lag:] = bi * aj - ai * bj
    return a, b, p, q, r_re, r_im


def fold(x, width):
    """fold_W over the last axis of x: `width` accumulators from +0.0, accumulator l adds x[l], x[l + W], ... in that order
    (one vectorised add per step), then acc[l] = acc[l] + acc[l ^ k] for k = 1, 2, ..., W / 2; acc[0].  An absent x is +0.0."""
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[-1]
    steps = -(-m // width)
    padded = np.zeros(x.shape[:-1] + (steps * width,))
    padded[..., :m] = x
    padded = padded.reshape(x.shape[:-1] + (steps, width))
    acc = np.zeros(x.shape[:-1] + (width,))
    for s in range(steps):
        acc = acc + padded[..., s, :]
    lanes = np.arange(width)
    k = 1
    while k < width:
        acc = acc + acc[..., lanes ^ k]
        k *= 2
    return acc[..., 0]


def job_sum(x):
    """One of the six sums of a job from its term array: fold_256 inside every tile of TILE pairs, fold_64 over the tiles."""
    x = np.asarray(x, dtype=np.float64)
    tiles = -(-x.size // TILE)
    if tiles == 0:
        return np.float64(0.0)
    padded = np.zeros(tiles * TILE)
    padded[:x.size] = x
    return fold(fold(padded.reshape(tiles, TILE), 256), 64)


def sums(pairs, offset=0j, lag=1):
    """The record of one job (a SUMS scalar): what fsea_measure_run_* writes for these pairs, bit for bit."""
    t = terms(pairs, offset, lag)
    n = t[0].size
    out = np.zeros((), dtype=SUMS)
    for name, x in zip(NAMES, t):
        out[name] = job_sum(x)
    p = np.where(np.isnan(t[2]), 0.0, t[2])         # a NaN term is never the peak
    if n:
        out["peak"] = p.max()
        out["peak_index"] = int(np.argmax(p))       # the first that has it
    out["n_pairs"] = n
    out["n_lagged"] = max(n - lag, 0)
    return out


def measure_jobs(extract_jobs, decimation, skip_pairs):
    """fsea_measure_jobs: (first_pair, n_pairs) per extract job (records with n_samples and out_first)."""
    out = np.zeros(len(extract_jobs), dtype=JOB)
    for k, j in enumerate(extract_jobs):
        outs = int(j.n_samples) // decimation
        skip = min(skip_pairs, outs)
        out[k] = (int(j.out_first) + skip, outs - skip)
    return out


def finish(s, lag=1):
    """fsea_measure_finish's formulas on a SUMS scalar -> dict; NaN where the header says so."""
    with np.errstate(all="ignore"):
        n, m = np.float64(int(s["n_pairs"])), np.float64(int(s["n_lagged"]))
        p = np.float64(s["p"])
        out = {"mean_power": p / n, "dc_re": s["s_re"] / n, "dc_im": s["s_im"] / n, "kurtosis": n * s["q"] / (p * p),
               "crest": s["peak"] * n / p, "peak_index": int(s["peak_index"]), "n_pairs": int(s["n_pairs"])}
        out["power_db"] = 10.0 * np.log10(out["mean_power"])
        out["freq_cycles"] = out["coherence"] = out["width_cycles"] = np.float64(np.nan)
        if m > 0:
            ratio = np.hypot(s["r_re"], s["r_im"]) * n / (p * m)
            out["freq_cycles"] = np.arctan2(s["r_im"], s["r_re"]) / (2.0 * np.pi * lag)
            out["coherence"] = np.float64(1.0) if ratio > 1.0 else ratio
            out["width_cycles"] = np.sqrt(-2.0 * np.log(out["coherence"]) + 0.0) / (2.0 * np.pi * lag)
    return out
