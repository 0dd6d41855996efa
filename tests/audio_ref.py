"""A numpy restatement of fsea_audio_*, written from the contract in include/fsea.h, not from the kernel: the terms of a job
in f64 with the header's roundings (numpy rounds every product, sum, quotient and square root on its own), the FM
discriminator branch by branch, the AM envelope, the filter as one vectorised multiply and add per tap in ascending order,
the last rounding to f32; the layout; the tile size the object picks (for the tests' choice of lengths only: no output
depends on it); and the synthetic FM and AM signals of the tests with the check they make of a demodulated tone."""
import math

import numpy as np

FM, AM = 0, 1
JOB = np.dtype([("first_pair", "<u8"), ("n_pairs", "<u8"), ("out_first", "<u8")])      # fsea_audio_job
C0, C1, C2 = 0.98419158358617365, 0.093485702629671305, 0.19556307900617517


def tile(decimation, n_taps):
    """T: the largest count up to 256 with T D + L - 1 <= 4096"""
    return min(256, (4096 - (n_taps - 1)) // decimation)


def terms(pairs, offset=0j):
    z = np.ascontiguousarray(pairs, dtype=np.complex64).ravel()
    offset = complex(offset)
    return z.real.astype(np.float64) - np.float64(offset.real), z.imag.astype(np.float64) - np.float64(offset.imag)


def arctangent(real, imag):
    """The header's FM expression on the two products, elementwise; +0.0 where both are zero."""
    real, imag = np.asarray(real, dtype=np.float64), np.asarray(imag, dtype=np.float64)
    minus = imag < 0
    imag = np.where(minus, -imag, imag)
    silent = (real == 0) & (imag == 0)
    eq = real == imag
    gt = ~eq & (real > imag)
    third = ~eq & ~gt
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        div = np.where(eq, 1.0, np.where(gt, imag, real) / np.where(gt, real, imag))
        ang = np.where(third, -math.pi / 2, 0.0)
        minus = np.where(third, ~minus, minus)
        v = ang + div / (C0 + div * (C1 + div * C2))
    return np.where(silent, 0.0, np.where(minus, -v, v))


def discriminator(pairs, kind, offset=0j):
    """d of one job: one f64 per pair."""
    a, b = terms(pairs, offset)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == AM:
            return np.sqrt(a * a + b * b)
        d = np.zeros(a.size)
        if a.size > 1:
            pa, pb, ca, cb = a[:-1], b[:-1], a[1:], b[1:]
            d[1:] = arctangent(pa * ca + pb * cb, pa * cb - ca * pb)
    return d


def audio(pairs, kind, taps, decimation, offset=0j, gain=1.0):
    """The float32 audio of one job: what fsea_audio_run_* writes for these pairs, bit for bit.  len(pairs) // decimation
    outputs."""
    c = np.asarray(taps, dtype=np.float64).ravel()
    d = discriminator(pairs, kind, offset)
    n_out = d.size // decimation
    d_ext = np.concatenate([np.zeros(c.size - 1), d])
    acc = np.zeros(n_out)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(c.size):
            acc = acc + c[k] * d_ext[k:k + n_out * decimation:decimation][:n_out]
        return (np.float64(gain) * acc).astype(np.float32)


def layout(n_pairs, decimation):
    """(out_first per job, total outputs): back to back in table order."""
    at, firsts = 0, []
    for n in n_pairs:
        firsts.append(at)
        at += int(n) // decimation
    return firsts, at


def nan_outputs(n_pairs, kind, n_taps, decimation, at):
    """The outputs of a job of n_pairs pairs that a NaN pair at index `at` of the job reaches when every tap is non-zero: it
    poisons d[at] and, for FM, d[at + 1] (d[0] is +0.0 whatever pair 0 holds); output j reads d[j D - (L - 1) .. j D]."""
    ds = [i for i in ((at, at + 1) if kind == FM else (at,)) if 0 <= i < n_pairs and not (kind == FM and i == 0)]
    out = set()
    for i in ds:
        for j in range(-(-i // decimation), (i + n_taps - 1) // decimation + 1):
            if j < n_pairs // decimation:
                out.add(j)
    return sorted(out)


# ---- the synthetic signals of the tests ------------------------------------------------------------------------------

def fm_signal(n, rate, tone, deviation, amplitude=1.0, phase0=0.3):
    """n complex samples at `rate` of a carrier at 0 Hz frequency-modulated by a cosine of `tone` Hz with `deviation` Hz peak:
    the instantaneous frequency is deviation cos(2 pi tone t)."""
    t = np.arange(n) / float(rate)
    return amplitude * np.exp(1j * (phase0 + (deviation / tone) * np.sin(2 * math.pi * tone * t)))


def am_signal(n, rate, tone, depth, amplitude=1.0, phase0=0.3):
    t = np.arange(n) / float(rate)
    return amplitude * (1.0 + depth * np.cos(2 * math.pi * tone * t)) * np.exp(1j * phase0)


def tone_fit(x, rate, tone):
    """(amplitude, mean, rms of the rest) of the least-squares fit of mean + A cos(2 pi tone t + phi) to x at `rate`."""
    x = np.asarray(x, dtype=np.float64)
    t = np.arange(x.size) / float(rate)
    basis = np.stack([np.ones(x.size), np.cos(2 * math.pi * tone * t), np.sin(2 * math.pi * tone * t)], axis=1)
    coef, *_ = np.linalg.lstsq(basis, x, rcond=None)
    rest = x - basis @ coef
    return float(np.hypot(coef[1], coef[2])), float(coef[0]), float(np.sqrt(np.mean(rest * rest)))
