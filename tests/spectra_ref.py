"""A numpy restatement of fsea_spectra_*, written from the contract in include/fsea.h, not from the kernels: the terms, the
kinds, the taper and the sign in float32 with the header's roundings (numpy rounds every product and every sum on its own),
then numpy.fft.fft in complex128 on those f32 inputs, |X|^2 in f64 and the average over the segments in f64;
fsea_spectra_segments, _layout, _jobs as their formulas and fsea_spectra_finish as a literal loop.  Plus the synthetic
emissions the tests look at: PSK bursts with a known symbol rate and carrier offset."""
import math

import numpy as np

Z, ENVELOPE, SQUARE, FOURTH = 0, 1, 2, 3
KINDS = (Z, ENVELOPE, SQUARE, FOURTH)
TILE_SEGMENTS = 32
JOB = np.dtype([("first_pair", "<u8"), ("n_pairs", "<u8"), ("out_first", "<u8")])        # fsea_spectra_job


def terms(pairs, offset=0j):
    """(a, b) of a job's pairs: the pedestal taken off in f64, then one rounding to f32."""
    z = np.ascontiguousarray(pairs, dtype=np.complex64).ravel()
    offset = complex(offset)
    a = (z.real.astype(np.float64) - np.float64(offset.real)).astype(np.float32)
    b = (z.imag.astype(np.float64) - np.float64(offset.imag)).astype(np.float32)
    return a, b


def square(a, b):
    return a * a - b * b, np.float32(2.0) * (a * b)


def kind_of(a, b, kind):
    """(u, v) of the kind, float32, every product and sum rounded on its own."""
    assert a.dtype == np.float32 and b.dtype == np.float32
    if kind == Z:
        return a, b
    if kind == ENVELOPE:
        return a * a + b * b, np.zeros_like(a)
    u, v = square(a, b)
    if kind == FOURTH:
        u, v = square(u, v)
    assert kind in (SQUARE, FOURTH)
    return u, v


def segments(n_pairs, n, hop):
    return 0 if n_pairs < n else (n_pairs - n) // hop + 1


def inputs(pairs, n, hop, kind, window=None, offset=0j):
    """x of every segment, (S, n) complex64: kind, taper, sign."""
    a, b = terms(pairs, offset)
    with np.errstate(all="ignore"):
        u, v = kind_of(a, b, kind)
    S = segments(u.size, n, hop)
    at = (np.arange(S) * hop)[:, None] + np.arange(n)[None, :]
    us, vs = u[at], v[at]
    if window is not None:
        w = np.ascontiguousarray(window, dtype=np.float32)
        assert w.shape == (n,)
        with np.errstate(all="ignore"):
            us, vs = w[None, :] * us, w[None, :] * vs
    sign = np.where(np.arange(n) % 2 == 1, np.float32(-1.0), np.float32(1.0))[None, :]
    x = np.empty((S, n), np.complex64)
    x.real, x.imag = sign * us, sign * vs
    return x


def segment_powers(pairs, n, hop, kind, window=None, offset=0j):
    """p_s[k] in f64 from an exact-to-f64 transform of the f32 inputs, (S, n)."""
    x = inputs(pairs, n, hop, kind, window, offset)
    with np.errstate(all="ignore"):
        X = np.fft.fft(x.astype(np.complex128), axis=1)
        return X.real * X.real + X.imag * X.imag


def spectrum(pairs, n, hop, kind, window=None, offset=0j):
    """(the n averaged powers in f64, or an empty array where the span has no segment; the bound's scale mean_s max_k p_s[k])"""
    p = segment_powers(pairs, n, hop, kind, window, offset)
    if p.shape[0] == 0:
        return np.zeros(0), 0.0
    total = np.zeros(n)
    for s in range(p.shape[0]):
        total = total + p[s]
    with np.errstate(all="ignore"):
        return total / np.float64(p.shape[0]), float(np.mean(np.max(p, axis=1)))


def layout(ns, n, hop):
    """fsea_spectra_layout: out_first per job and the floats in all."""
    at, firsts = 0, []
    for m in ns:
        firsts.append(at)
        at += n if segments(m, n, hop) else 0
    return firsts, at


def spectra_jobs(extract_jobs, decimation, skip_pairs):
    """fsea_spectra_jobs: (first_pair, n_pairs, 0) per extract job (records with n_samples and out_first)."""
    out = np.zeros(len(extract_jobs), dtype=JOB)
    for k, j in enumerate(extract_jobs):
        outs = int(j.n_samples) // decimation
        skip = min(skip_pairs, outs)
        out[k] = (int(j.out_first) + skip, outs - skip, 0)
    return out


def finish(power, guard_bins, fraction):
    """fsea_spectra_finish as the header words it, one loop after the other, all in f64 -> dict."""
    P = [float(v) for v in np.asarray(power, dtype=np.float32)]
    n = len(P)
    half = n // 2
    nan = float("nan")
    total = 0.0
    moment = 0.0
    for k in range(n):
        total += P[k]
        moment += float(k - half) * P[k]
    out = {"total": total, "centroid_cycles": (moment / total / n) if total != 0.0 else nan}
    t = total * (1.0 - fraction) / 2.0
    c, lo, hi = 0.0, -1, -1
    for k in range(n):
        c += P[k]
        if lo < 0 and c > t:
            lo = k
        if hi < 0 and c >= total - t:
            hi = k
    if lo < 0 or hi < 0:
        lo = hi = -1
    out.update(obw_lo=lo, obw_hi=hi, obw_bins=hi - lo + 1 if lo >= 0 else 0,
               obw_centre_cycles=((lo + hi) / 2.0 - half) / n if lo >= 0 else nan)
    rest = [k for k in range(n) if abs(k - half) > guard_bins]
    peak_bin = rest[0]
    for k in rest:
        if P[k] > P[peak_bin]:
            peak_bin = k
    ordered = sorted(P[k] for k in rest)
    floor = ordered[(len(ordered) - 1) // 2]
    with np.errstate(all="ignore"):
        line_db = float(10.0 * np.log10(np.float64(P[peak_bin]) / np.float64(floor)))
    out.update(peak_bin=peak_bin, peak_power=P[peak_bin], peak_cycles=(peak_bin - half) / n, floor=floor, line_db=line_db)
    return out


# ---- synthetic emissions ------------------------------------------------------------------------------------------------

def psk(n, order, pairs_per_symbol, carrier_cycles, amplitude=1.0, seed=1, shaped=True):
    """n pairs of `order`-PSK (2: BPSK, 4: QPSK) at pairs_per_symbol pairs a symbol, carrier_cycles cycles per pair off the
    centre.  shaped: every symbol under a half-sine pulse, so the envelope has a line at the symbol rate (a rectangular
    pulse has a constant envelope and none)."""
    rng = np.random.default_rng(seed)
    symbols = rng.integers(0, order, -(-n // pairs_per_symbol))
    phase = np.repeat(2.0 * np.pi * symbols / order + (np.pi / 4 if order == 4 else 0.0), pairs_per_symbol)[:n]
    t = np.arange(n)
    pulse = np.sin(np.pi * ((t % pairs_per_symbol) + 0.5) / pairs_per_symbol) if shaped else 1.0
    return amplitude * pulse * np.exp(1j * phase) * np.exp(2j * np.pi * carrier_cycles * t)


def qpsk_cutout(n, seed=7, carrier_cycles=0.03125, noise=0.05, pedestal=0.5 + 0.5j):
    """The synthetic cut-out of the GPU tier: QPSK at 8 pairs a symbol plus noise on the cut-outs' pedestal, complex64."""
    rng = np.random.default_rng(seed)
    w = noise * (rng.normal(0.0, 1.0, n) + 1j * rng.normal(0.0, 1.0, n))
    return (psk(n, 4, 8, carrier_cycles, 1.0, seed) + w + pedestal).astype(np.complex64)


def noise_cutout(n, seed=8, pedestal=0.5 + 0.5j):
    """Noise alone: no bin dominates."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 1.0, n) + 1j * rng.normal(0.0, 1.0, n) + pedestal).astype(np.complex64)


# ---- inputs whose spectra have a closed form that f32 gives exactly ---------------------------------------------------------------

CONSTANT, IMPULSE = 2.0 - 0.25j, 4.0 - 2.0j       # halves and quarters: every term, square and fourth power is exact in f32


def constant_pairs(m, offset=0j):
    """m pairs that are all offset + CONSTANT"""
    return np.full(m, complex(offset) + CONSTANT, np.complex64)


def impulse_pairs(n, offset=0j):
    """one segment: pair 0 is offset + IMPULSE, every other pair the offset alone"""
    z = np.full(n, complex(offset), np.complex64)
    z[0] = complex(offset) + IMPULSE
    return z


def constant_spectrum(n, kind, dtype=np.float32):
    """The n powers of constant_pairs without a taper, any S and hop: x_j = (-1)^j (u, v), so X is n (u, v) in bin n / 2 and
    +0 in every other.  (u, v) is kind_of in f32; with dtype float32 the power is n^2 (u u + v v) as f32 arithmetic rounds
    it, which is what a transform that multiplies by no twiddle but 1 gives; with float64 it is the exact value."""
    u, v = kind_of(np.float32([CONSTANT.real]), np.float32([CONSTANT.imag]), kind)
    u, v = dtype(u[0]), dtype(v[0])
    want = np.zeros(n, dtype)
    want[n // 2] = dtype(n) * dtype(n) * (u * u + v * v)
    return want


def impulse_spectrum(n, dtype=np.float32):
    """The n powers of impulse_pairs, kind Z, no taper: X[k] = IMPULSE for every k, |4 - 2i|^2 = 20"""
    return np.full(n, IMPULSE.real ** 2 + IMPULSE.imag ** 2, dtype)


def nan_bins(n_pairs, n, hop, at):
    """The bins of a job's output that a NaN in its pair `at` reaches: all n where a segment covers the pair, none otherwise."""
    S = segments(n_pairs, n, hop)
    covered = any(s * hop <= at < s * hop + n for s in range(S))
    return list(range(n)) if covered else []


def hann(n):
    """the periodic Hann taper in f32, the formula alone"""
    return (0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(n) / n)).astype(np.float32)
