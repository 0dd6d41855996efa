"""A numpy f64 restatement of the reference's audio chain (src/nrf.c:654-676, 778-811, 904-1094): the low-pass design,
the downsampler with its accumulated floor(t) indices, the RAW and WBFM demodulators and the decoder.  The tests hold it
against the reference's recorded outputs (tests/golden/demod_golden.npz) and the GPU against it."""
import math

import numpy as np

INTER_RATE, MAX_F = 336000, 75000
TAU = math.pi * 2


def lowpass_taps(rate, cutoff, length):
    """nrf_fir_get_low_pass_coefficients: the first `length` of the m = length + (length + 1) % 2 designed taps."""
    m = length + (length + 1) % 2
    f = cutoff / rate
    c = m // 2
    v = np.empty(m)
    for i in range(m):
        if i == c:
            x = TAU * f
        else:
            a = TAU * (i + 1) / float(m + 1)
            x = math.sin(TAU * f * (i - c)) / float(i - c)
            x *= 0.42 - 0.5 * math.cos(a) + 0.08 * math.cos(2 * a)
        v[i] = x
    s = 0.0
    for x in v:
        s += x
    return (v / s)[:length]


def out_length(n, rate_mul):
    return int(math.floor(n / rate_mul))


def index_table(n, rate_mul):
    """The reference's idx_j = floor(t_j), t accumulated (t += rate_mul) from 0."""
    count = out_length(n, rate_mul)
    steps = np.full(count, rate_mul)
    if count:
        steps[0] = 0.0
    return np.floor(np.add.accumulate(steps)).astype(np.int64)


class Downsampler:
    def __init__(self, in_rate, out_rate, cutoff, length):
        self.c = lowpass_taps(in_rate, cutoff, length)
        self.rate_mul = in_rate / float(out_rate)
        self.tail = np.zeros(length - 1)

    def process(self, x):
        L = self.c.size
        xe = np.concatenate([self.tail, np.asarray(x, dtype=np.float64)])
        self.tail = xe[xe.size - (L - 1):] if L > 1 else np.zeros(0)
        idx = index_table(len(x), self.rate_mul)
        if idx.size == 0:
            return np.zeros(0)
        win = np.lib.stride_tricks.sliding_window_view(xe, L)[idx]
        return win @ self.c


def discriminate(li, lq, yi, yq, ampl_conv):
    """src/nrf.c:969-993, elementwise: (li, lq) the previous stage-1 output, (yi, yq) the current one."""
    real = li * yi + lq * yq
    imag = li * yq - yi * lq
    neg = imag < 0
    sgn = np.where(neg, -1.0, 1.0)
    imag = np.where(neg, -imag, imag)
    eq = real == imag
    gt = ~eq & (real > imag)
    el = ~eq & ~gt
    with np.errstate(divide="ignore", invalid="ignore"):
        div = np.where(eq, 1.0, np.where(gt, imag / real, real / imag))
    ang = np.where(el, -math.pi / 2, 0.0)
    sgn = np.where(el, -sgn, sgn)
    return sgn * (ang + div / (0.98419158358617365 + div * (0.093485702629671305 + div * 0.19556307900617517))) * ampl_conv


class RawDemodulator:
    def __init__(self, in_rate, out_rate):
        self.ds = Downsampler(in_rate, out_rate, out_rate // 2, 41)

    def process(self, i, q):
        return self.ds.process(i)


class FmDemodulator:
    def __init__(self, in_rate, out_rate):
        self.ds_i = Downsampler(in_rate, INTER_RATE, int(MAX_F * 0.8), 51)
        self.ds_q = Downsampler(in_rate, INTER_RATE, int(MAX_F * 0.8), 51)
        self.ds_audio = Downsampler(INTER_RATE, out_rate, 10000, 41)
        self.ampl_conv = out_rate / (TAU * MAX_F)
        self.alpha = 1.0 / (1.0 + out_rate * 50.0 / 1e6)
        self.l = (0.0, 0.0)
        self.val = 0.0

    def process(self, i, q):
        yi, yq = self.ds_i.process(i), self.ds_q.process(q)
        if yi.size:
            li = np.concatenate([[self.l[0]], yi[:-1]])
            lq = np.concatenate([[self.l[1]], yq[:-1]])
            d = discriminate(li, lq, yi, yq, self.ampl_conv)
            self.l = (yi[-1], yq[-1])
        else:
            d = np.zeros(0)
        a = self.ds_audio.process(d)
        out = np.empty_like(a)
        val, alpha = self.val, self.alpha
        for k, x in enumerate(a.tolist()):
            val = val + alpha * (x - val)
            out[k] = val
        self.val = val
        return out


def convert(u8):
    """The decoder's conversion of offset-binary bytes: b / 128.0 - 0.995."""
    return np.asarray(u8).astype(np.float64) / 128.0 - 0.995


def rotate_reference(i, q, offset, rate, c, s):
    """nrf_freq_shifter_process_samples: the running-product phase, sample by sample (returns i', q', c, s)."""
    dc, ds = math.cos(TAU * offset / float(rate)), math.sin(TAU * offset / float(rate))
    oi, oq = np.empty(len(i)), np.empty(len(i))
    for k, (vi, vq) in enumerate(zip(i.tolist(), q.tolist())):
        oi[k] = vi * c - vq * s
        oq[k] = vi * s + vq * c
        c, s = c * dc - s * ds, c * ds + s * dc
    return oi, oq, c, s


def rotate_exact(i, q, offset, rate, c, s):
    """The rotation with the phase of sample k from the exactly reduced cycle count (offset k mod rate) / rate."""
    n = len(i)
    m = (offset % rate) * (np.arange(n, dtype=np.int64) % rate) % rate
    ph = (c + 1j * s) * np.exp(1j * TAU * (m / float(rate)))
    z = (np.asarray(i) + 1j * np.asarray(q)) * ph
    mn = (offset % rate) * (n % rate) % rate
    e = (c + 1j * s) * complex(math.cos(TAU * mn / float(rate)), math.sin(TAU * mn / float(rate)))
    return z.real.copy(), z.imag.copy(), e.real, e.imag


class Decoder:
    """nrf_decoder: kind 0 RAW, 1 WBFM; phase="reference" (the running product) or "exact" (this project's)."""

    def __init__(self, kind, in_rate, out_rate, offset, phase="reference"):
        self.dm = RawDemodulator(in_rate, out_rate) if kind == 0 else FmDemodulator(in_rate, out_rate)
        self.rate, self.offset, self.c, self.s = in_rate, offset, 1.0, 0.0
        self.rotate = rotate_reference if phase == "reference" else rotate_exact

    def process(self, u8):
        u8 = np.asarray(u8, dtype=np.uint8)
        i, q = convert(u8[0::2]), convert(u8[1::2])
        i, q, self.c, self.s = self.rotate(i, q, self.offset, self.rate, self.c, self.s)
        return self.dm.process(i, q)


def pcm(audio):
    """(int16_t)(audio * 32000)."""
    return np.trunc(np.asarray(audio) * 32000).astype(np.int16)
