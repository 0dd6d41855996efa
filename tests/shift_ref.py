"""The shifted paths (fsea_fir_u8_shifted_*, fsea_chain_* with a shift, fsea_zoom_*) restated with an exact phase, in plain
Python and numpy, for every stream position the forms accept.

tests/test_iq_chain_host.py's shifted_samples forms phase0 + (offset + m) * delta as one rounded double product; against
exact arithmetic that is off by 2.6e-8 cycles at position 2^31 and by 1e-5 at 2^40 (delta = -0.12): good up to about 2^24
and no judge beyond.  Here a double delta is the exact rational it is (float.as_integer_ratio: an integer over a power of
two), the phase of stream position P is

    frac(p0 + delta * P),   p0 = phase0 - floor(phase0) as make_rot (fsea_fir_stage.h) forms it in double,

computed in Python integers and rounded to f64 once, by the one division at the end.  p0 is the library's own reduction
of phase0_cycles on purpose: it is part of the documented arithmetic ("reduced modulo 1 together with phase0_cycles"), and
for the values the tests use it equals the exact frac(phase0) (tests/test_shift_ref_host.py shows that), so the two readings
do not differ there.  From the phase on: x * e^{2 pi i turns} + 0.5 (1 + i), fir_reference of tests/test_fir_host.py, every
D-th output for the zoom, n_zero samples of 0.0 behind the block for the chain.

A few thousand samples per case: the per-sample big-integer arithmetic costs milliseconds."""
import functools
import math

import numpy as np

from tests.test_fir_host import fir_reference


def reduced_phase0(phase0):
    """phase0 - floor(phase0) in double: make_rot's r.phase0."""
    return float(phase0) - math.floor(float(phase0))


def _over_pow2(x):
    """A finite double as (numerator, log2 of the denominator)."""
    num, den = float(x).as_integer_ratio()
    assert den & (den - 1) == 0
    return num, den.bit_length() - 1


def exact_turns_fraction(delta, phase0, P):
    """frac(p0 + delta * P) of one stream position as (numerator, denominator), exact."""
    dn, dk = _over_pow2(delta)
    pn, pk = _over_pow2(reduced_phase0(phase0))
    k = max(dk, pk)
    den = 1 << k
    return ((pn << (k - pk)) + (dn << (k - dk)) * int(P)) % den, den


@functools.lru_cache(maxsize=None)
def exact_turns(delta, phase0, offset, n):
    """The phases, in [0, 1] cycles, of the stream positions offset .. offset + n - 1: exact, then rounded to f64 once.
    Computed once per argument tuple and shared: the array is read-only."""
    dn, dk = _over_pow2(delta)
    pn, pk = _over_pow2(reduced_phase0(phase0))
    k = max(dk, pk)
    den, step = 1 << k, dn << (k - dk)
    at = ((pn << (k - pk)) + step * int(offset)) % den
    out = np.empty(n, dtype=np.float64)
    for m in range(n):
        out[m] = at / den            # int / int: correctly rounded
        at += step
        at %= den
    out.flags.writeable = False
    return out


def u8_pairs(u8, flip):
    b = np.asarray(u8, dtype=np.uint8)
    b = b ^ 0x80 if flip else b
    return b[0::2] / 256.0 + 1j * (b[1::2] / 256.0)


def shifted_samples(u8, flip, delta, phase0, offset=0):
    """Sample m of the call, at stream position offset + m: (u8 / 256) e^{2 pi i turns} + 0.5 (1 + i), turns exact."""
    x = u8_pairs(u8, flip)
    return x * np.exp(2j * np.pi * exact_turns(delta, phase0, offset, x.size)) + (0.5 + 0.5j)


def shifted_fir_reference(u8, flip, delta, phase0, taps, tail=None, offset=0, n_zero=0):
    """The shifted filter in f64: the rotated block, n_zero samples of plain 0.0 behind it (the chain), through
    fir_reference.  Returns (y, next tail)."""
    x = np.concatenate([shifted_samples(u8, flip, delta, phase0, offset), np.zeros(n_zero, dtype=np.complex128)])
    return fir_reference(x, taps, tail)


def zoom_reference(u8, flip, delta, phase0, taps, D, tail=None, offset=0):
    """The decimating filter: outputs 0, D, 2 D, ... of the full-rate filter, n // D of them; the tail is the full-rate
    filter's.  Returns (pairs, next tail)."""
    y, tail = shifted_fir_reference(u8, flip, delta, phase0, taps, tail, offset=offset)
    return y[::D][:y.size // D], tail


def chain_frames_reference(u8, n, n_frames, flip, delta, phase0, taps, offset=0, n_zero=0, tail=None):
    """n_frames consecutive blocks of n pairs, each followed by n_zero zeros through the filter; frame f stands at stream
    position offset + f n (the zeros are no samples of the stream).  Returns ((n_frames, n + n_zero) pairs, next tail)."""
    u8 = np.asarray(u8, dtype=np.uint8)
    frames = []
    for f in range(n_frames):
        y, tail = shifted_fir_reference(u8[2 * n * f:2 * n * (f + 1)], flip, delta, phase0, taps, tail, offset + f * n, n_zero)
        frames.append(y)
    return np.stack(frames), tail
