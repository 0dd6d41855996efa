"""CPU tier: the exact-phase reference of the shifted paths (tests/shift_ref.py) and what can be said about those paths
without a GPU --
  - the exact reference agrees with the older restatement (tests/test_iq_chain_host.py: one rounded double product) where
    that one's own rounding allows, and with the reference's recorded dvbt.lua chain; at position 2^44 the two differ by
    more than 1e-5 cycles, which is why the exact one exists;
  - rot_base of fsea_fir_stage.h restated line by line (Python floats are IEEE doubles, the fma residual exact from
    Fraction) stays within 2^-30 cycles of the exact phase over the whole argument domain;
  - fsea_chain_run_host / _device refuse bad shift arguments before they touch the object, and with shift == 0 do not look
    at them.

The cap on the reduction, 2^-30 cycles (cyclic distance), is derived, not measured: the kernel rounds the reduced phase to
float next, (float)t, which adds up to 2^-25; 1/32 of that leaves the phasor error budget of tests/test_gpu_iq_chain.py ("a
few 2^-24") untouched at every position, so MAX_ABS and MAX_REL of tests/test_gpu_fir.py keep their derivation.  Measured
worst (printed by the test, recorded in DESIGN.md section 6): 2^-52.4 for |cps| <= 0.5, 2^-36.0 for |cps| <= 2^20.

The restatement is of the source text.  Whether the compiled kernel computes it is the GPU tier's question
(tests/test_gpu_shift_domain.py): it did not, a contraction had counted the fma residual twice."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import shift_ref
from tests.conftest import ROOT
from tests.test_fir_host import GOLDEN
from tests.test_gpu_iq_chain import CYCLES, PHASES
from tests.test_iq_chain_host import shifted_samples as product_samples

FSEA_EINVAL = -1
LIMIT = 1 << 52

# the grid of tests/test_gpu_shift_domain.py
GRID_CYCLES = [-1.2e6 / 10e6, 0.4999, 0.5, 1.0, 2.0 ** 20, -2.0 ** 20, 1048575.999, -881917.8337624283, 1e-12, 2.0 ** -40,
               5e-324, -0.0]
GRID_PHASES = [0.0, 0.75, -12345.678, 1e15, -2.0 ** 52]
GRID_N = 2 * 2048 + 13


def grid_positions(n=GRID_N):
    """sample_offset of a call of n samples: 0, across 2^24, 2^31 and 2^32 (2^32 inside the call and inside a tile), above
    2^40, and the last admissible call."""
    return [0, (1 << 24) - 3, (1 << 31) - 5, (1 << 32) - 2053, (1 << 40) + 3, LIMIT - n]


def cyclic(a, b):
    """The distance of two phases on the circle, as a Fraction."""
    d = (Fraction(a) - Fraction(b)) % 1
    return min(d, 1 - d)


def recovered_turns(samples, x):
    """The phase a restatement rotated x by, from its samples x e^{2 pi i turns} + 0.5 (1 + i): good to ~1e-16."""
    return np.angle((samples - (0.5 + 0.5j)) / x) / (2.0 * np.pi)


def bright_bytes(n, seed):
    """Interleaved bytes with I >= 128: |u8 / 256| >= 0.5, so the phase is recoverable from a sample."""
    iq = np.random.default_rng(seed).integers(0, 256, 2 * n, dtype=np.uint8)
    iq[0::2] |= 0x80
    return iq


# ---- the reference itself -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase0", GRID_PHASES + PHASES)
def test_make_rots_phase0_reduction_is_exact_for_the_phases_used(phase0):
    """phase0 - floor(phase0) in double (make_rot, and the reference here) against frac(phase0) in rationals: equal for
    every phase0 the tests use, so "reduced as make_rot" and "exact" are one reading for them."""
    exact = Fraction(phase0) - math.floor(Fraction(phase0))
    assert Fraction(shift_ref.reduced_phase0(phase0)) == exact and 0 <= exact < 1


def test_exact_turns_are_the_rational_phase_rounded_once():
    """The vector form steps an integer numerator; against the one-position form and against Fraction directly."""
    for delta, phase0, offset in ((-0.12, 0.75, (1 << 44) + 5), (5e-324, 0.0, LIMIT - 9), (1048575.999, -12345.678, (1 << 32) - 4)):
        got = shift_ref.exact_turns(delta, phase0, offset, 9)
        for m in range(9):
            want = (Fraction(shift_ref.reduced_phase0(phase0)) + Fraction(delta) * (offset + m)) % 1
            num, den = shift_ref.exact_turns_fraction(delta, phase0, offset + m)
            assert Fraction(num, den) == want and got[m] == float(want), (delta, phase0, offset, m)
    # a delta of 1 / 100 is not a double; the double next to it is what the library is given and what is exact here
    assert shift_ref.exact_turns(0.25, 0.0, 3, 1)[0] == 0.75 and shift_ref.exact_turns(-0.25, 0.5, LIMIT - 1, 1)[0] == 0.75


def product_bound(delta, phase0, last):
    """The older restatement's own rounding up to stream position `last`, in cycles: half an ulp of the product
    (offset + m) delta and half an ulp of its sum with phase0 (the subtraction of the floor is exact)."""
    product = abs(delta) * last
    return (math.ulp(product) + math.ulp(product + abs(phase0))) / 2 if product + abs(phase0) else 0.0


@pytest.mark.parametrize("phase0", PHASES)
@pytest.mark.parametrize("cps", CYCLES)
def test_exact_reference_agrees_with_the_product_restatement_where_that_one_is_good(cps, phase0):
    """1e-12 cycles, cyclic distance, at every offset below 2^20 at which the product restatement's own rounding
    (product_bound) stays inside 1e-12: always offsets 0 and 3; how far up depends on |cps| and phase0 -- at phase0 =
    12345.678 half an ulp of the sum is 9.1e-13 already, which leaves room for products below 512."""
    n, used = 64, []
    iq = bright_bytes(n, 1)
    x = shift_ref.u8_pairs(iq, 0)
    for offset in (0, 3, 1000, (1 << 13) - 3, (1 << 16) + 5, (1 << 20) - 1 - n):
        if product_bound(cps, phase0, offset + n) > 1e-12:
            continue
        used.append(offset)
        old = recovered_turns(product_samples(iq, 0, cps, phase0, offset), x)
        new = shift_ref.exact_turns(cps, phase0, offset, n)
        worst = max(cyclic(float(a), float(b)) for a, b in zip(old, new))
        assert worst <= 1e-12, (cps, phase0, offset, float(worst))
        # and the samples themselves: |x| < 1.42, so 2 pi 1.42 times that
        dev = float(np.max(np.abs(product_samples(iq, 0, cps, phase0, offset) - shift_ref.shifted_samples(iq, 0, cps, phase0, offset))))
        assert dev <= 2 * np.pi * 1.42 * 1e-12, (cps, phase0, offset, dev)
    print("cps %r phase0 %r: offsets %r" % (cps, phase0, used))
    assert used[:2] == [0, 3] and (cps != 0.0 or len(used) == 6)


def test_exact_reference_reproduces_the_references_dvbt_chain():
    """Three steps of lua/dvbt.lua's shifter -> filter(5e6, 60e3, 97) as the reference recorded them, at the 1e-9 of
    tests/test_iq_chain_host.py's test of the product restatement."""
    with np.load(GOLDEN) as z:
        gold = {k: z[k] for k in z.files}
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        block = z["block__raw"] ^ 0x80
    n = block.size // 2
    delta = float(gold["dvbt__shift"]) / 5e6
    c = gold["taps__5000000_60000_97"]
    idx, tail = gold["dvbt__index"], None
    for step in range(3):
        y, tail = shift_ref.shifted_fir_reference(block, 0, delta, 0.0, c, tail, offset=step * n, n_zero=n)
        want = gold["dvbt__out"][step]
        dev = float(np.max(np.abs(y[idx] - (want[:, 0] + 1j * want[:, 1]))))
        print("step %d: max deviation %.3e" % (step, dev))
        assert y.size == 2 * n and dev < 1e-9, (step, dev)


def test_the_product_restatement_is_no_judge_at_2_to_the_44():
    """Why tests/shift_ref.py exists: at offset 2^44, delta = -1.2e6 / 10e6 the single rounded product is more than 1e-5
    cycles from the exact phase (its half ulp there is 2.4e-4).  If this stops failing the product restatement, the exact
    reference has become as weak as that one."""
    n, offset, delta = 64, 1 << 44, -1.2e6 / 10e6
    iq = bright_bytes(n, 2)
    x = shift_ref.u8_pairs(iq, 0)
    old = recovered_turns(product_samples(iq, 0, delta, 0.0, offset), x)
    new = shift_ref.exact_turns(delta, 0.0, offset, n)
    direct = [float((Fraction(delta) * (offset + m)) % 1) for m in range(n)]       # no code of shift_ref at all
    assert np.array_equal(new, direct)
    worst = float(max(cyclic(float(a), float(b)) for a, b in zip(old, new)))
    print("product restatement against the exact phase at 2^44: %.3e cycles" % worst)
    assert 1e-5 < worst < 2.5e-4, worst


# ---- the kernel's reduction, restated -------------------------------------------------------------------------------

def rot_base_turns(delta, p0, P):
    """fsea_fir_stage.h: rot_base up to the float conversion, line by line.  p0 = make_rot's r.phase0."""
    k = float(P)                                                # const double k = (double)P;         (P <= 2^52: exact)
    hi = delta * k                                              # const double hi = __dmul_rn(r.delta, k);
    lo = float(Fraction(delta) * Fraction(k) - Fraction(hi))    # const double lo = fma(r.delta, k, -hi);   one rounding
    t = (hi - math.floor(hi)) + (lo + p0)                       # double t = (hi - floor(hi)) + (lo + r.phase0);
    t -= math.floor(t)                                          # t -= floor(t);
    return t


def reduction_error(delta, phase0, P):
    num, den = shift_ref.exact_turns_fraction(delta, phase0, P)
    return cyclic(rot_base_turns(delta, shift_ref.reduced_phase0(phase0), P), Fraction(num, den))


def test_the_fma_residual_of_the_restatement_is_exact_where_it_is_representable():
    """hi + lo == delta * P exactly (the two-term product the header speaks of), away from underflow."""
    for delta, P in ((-0.12, (1 << 44) + 1), (1048575.999, LIMIT - 1), (2.0 ** -40, (1 << 32) + 7), (0.4999, 123456789)):
        hi = delta * float(P)
        lo = float(Fraction(delta) * P - Fraction(hi))
        assert Fraction(hi) + Fraction(lo) == Fraction(delta) * P and abs(lo) <= math.ulp(hi) / 2


def test_the_kernels_phase_reduction_stays_within_2_to_the_minus_30_of_the_exact_phase():
    cap = Fraction(1, 1 << 30)
    worst = {"|cps| <= 0.5": Fraction(0), "|cps| <= 2^20": Fraction(0)}

    def see(delta, phase0, P):
        e = reduction_error(delta, phase0, P)
        assert e <= cap, (delta, phase0, P, float(e))
        for name, top in (("|cps| <= 0.5", 0.5), ("|cps| <= 2^20", 2.0 ** 20)):
            if abs(delta) <= top:
                worst[name] = max(worst[name], e)

    # the grid of the GPU tier: the first and last sample of each call, the 8-sample bases either side, 2^32 itself
    for offset in grid_positions():
        inside = {offset, offset + 1, offset + GRID_N - 1, offset & ~7, (offset & ~7) + 8, (offset + GRID_N - 1) & ~7}
        if offset < (1 << 32) < offset + GRID_N:
            inside |= {(1 << 32) - 1, 1 << 32}
        for P in sorted(inside):
            for delta in GRID_CYCLES:
                for phase0 in GRID_PHASES:
                    see(delta, phase0, P)
    # a seeded sweep of the whole domain: |cps| <= 2^20 uniform and log-uniform, P in [0, 2^52] uniform, log-uniform and
    # in the top binade (where the residual is largest), phase0 in [0, 1)
    rng = np.random.default_rng(20)
    for i in range(20000):
        kind = i % 4
        if kind == 0:
            delta = float(rng.uniform(-2.0 ** 20, 2.0 ** 20))
        elif kind == 1:
            delta = float(rng.uniform(-0.5, 0.5))
        elif kind == 2:
            delta = float(np.ldexp(rng.uniform(0.5, 1.0), int(rng.integers(-60, 21)))) * (1 if rng.random() < 0.5 else -1)
        else:
            delta = float(np.nextafter(2.0 ** 20, 0.0) * rng.uniform(0.99, 1.0)) * (1 if rng.random() < 0.5 else -1)
        where = (i // 4) % 3
        if where == 0:
            P = int(rng.integers(0, LIMIT, endpoint=True))
        elif where == 1:
            P = int(rng.integers(1 << 51, LIMIT, endpoint=True))
        else:
            P = int(rng.integers(0, 1 << int(rng.integers(1, 53))))
        see(delta, float(rng.random()), P)
    see(2.0 ** 20, 0.0, LIMIT), see(-2.0 ** 20, 0.999, LIMIT), see(0.5, 0.0, LIMIT), see(-0.5, 0.75, LIMIT - 1)
    for name, e in worst.items():
        print("phase reduction, %s: worst 2^%.1f cycles" % (name, math.log2(e)))
    # the two statements of the corrected comments
    assert worst["|cps| <= 0.5"] <= Fraction(1, 1 << 50) and worst["|cps| <= 2^20"] <= Fraction(1, 1 << 35)


# ---- the chain's refusals -------------------------------------------------------------------------------------------

def _stage(shift, cps=0.01, phase0=0.0, offset=0, n_zero=0):
    return fsea.ChainStage(0, shift, cps, phase0, offset, n_zero)


BAD_SHIFTS = [(b"cycles_per_sample", dict(cps=np.nan)), (b"cycles_per_sample", dict(cps=np.inf)),
              (b"cycles_per_sample", dict(cps=-np.inf)), (b"cycles_per_sample", dict(cps=2.0 ** 21)),
              (b"phase0_cycles", dict(phase0=np.nan)), (b"phase0_cycles", dict(phase0=-np.inf)),
              (b"sample_offset", dict(offset=LIMIT + 1)), (b"sample_offset", dict(offset=LIMIT - 7))]


def _fake_object():
    """Zeroed memory in place of an object: a check that comes before the object is touched never reads it."""
    fake = ctypes.create_string_buffer(4096)
    return fake, ctypes.cast(fake, ctypes.c_void_p)


@pytest.mark.parametrize("n_zero", [0, 8])
@pytest.mark.parametrize("name,bad", BAD_SHIFTS)
def test_chain_refuses_bad_shift_arguments_before_it_touches_the_object(name, bad, n_zero):
    L = fsea.hip_lib()
    keep, f = _fake_object()
    buf = np.zeros(256, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    st = _stage(1, n_zero=n_zero, **bad)
    assert L.fsea_chain_run_host(f, p, 8, ctypes.byref(st), None) == FSEA_EINVAL, bad
    assert name in L.fsea_last_error_string(), (bad, L.fsea_last_error_string())
    for n_frames in (1, 3):
        assert L.fsea_chain_run_device(f, p, 8, n_frames, ctypes.byref(st), None, None) == FSEA_EINVAL, (bad, n_frames)
        assert name in L.fsea_last_error_string(), (bad, n_frames, L.fsea_last_error_string())
    assert keep.raw == bytes(4096)


@pytest.mark.parametrize("n_zero", [0, 2])
def test_chain_refuses_a_call_whose_last_frame_passes_the_limit(n_zero):
    """Three frames of 8 samples from 2^52 - 16: frames 0 and 1 end at or below 2^52, frame 2 does not.  The whole call is
    refused, before the object is touched -- not the third launch after two were queued."""
    L = fsea.hip_lib()
    keep, f = _fake_object()
    buf = np.zeros(256, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    st = _stage(1, offset=LIMIT - 16, n_zero=n_zero)
    assert L.fsea_chain_run_device(f, p, 8, 3, ctypes.byref(st), None, None) == FSEA_EINVAL
    assert b"sample_offset" in L.fsea_last_error_string()
    assert keep.raw == bytes(4096)


def test_chain_admits_the_last_call_and_ignores_the_shift_fields_without_a_shift():
    """As far as a fake pointer allows: each call here is refused by a LATER check (the outputs), whose text shows that the
    stage's check had nothing to say.  The last admissible calls: sample_offset + n_frames n_samples == 2^52, the zero
    samples not counted.  shift == 0: NaN, infinities and a position beyond the limit in the other fields are not looked
    at.  (tests/test_gpu_shift_domain.py runs both for real.)"""
    L = fsea.hip_lib()
    keep, f = _fake_object()
    buf = np.zeros(256, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    bad_host = fsea.ChainOutputs(None, p, 0, 0, None)                 # size_multiplier 0
    bad_device = fsea.ChainOutputs(p + 8, None, 1, 0, None)           # a misaligned device output
    stages = [(_stage(1, offset=LIMIT - 8, n_zero=8), 1), (_stage(1, offset=LIMIT - 24, n_zero=2), 3),
              (_stage(1, cps=2.0 ** 20, phase0=-2.0 ** 52, offset=LIMIT - 24), 3)]
    stages += [(_stage(0, **bad), 3) for _, bad in BAD_SHIFTS]
    for st, n_frames in stages:
        what = (st.shift, st.cycles_per_sample, st.phase0_cycles, st.sample_offset, st.n_zero, n_frames)
        if n_frames == 1:
            assert L.fsea_chain_run_host(f, p, 8, ctypes.byref(st), ctypes.byref(bad_host)) == FSEA_EINVAL, what
            assert b"size_multiplier" in L.fsea_last_error_string(), (what, L.fsea_last_error_string())
        assert L.fsea_chain_run_device(f, p, 8, n_frames, ctypes.byref(st), ctypes.byref(bad_device), None) == FSEA_EINVAL, what
        assert b"aligned" in L.fsea_last_error_string(), (what, L.fsea_last_error_string())
    st = _stage(0, cps=np.nan, phase0=np.inf, offset=LIMIT + 1)
    assert L.fsea_chain_run_host(f, p, 8, ctypes.byref(st), ctypes.byref(bad_host)) == FSEA_EINVAL
    assert b"size_multiplier" in L.fsea_last_error_string()
    assert keep.raw == bytes(4096)
