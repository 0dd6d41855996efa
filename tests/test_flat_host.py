"""CPU tier: the flat-spectrum input families of tests/flat_ref.py -- that they are what they claim, the kernel source on
them through tests/emu, and the teeth of the comparison.

Why the file exists (test_a_small_turn_fails_on_flat_frames_and_passes_on_synth_iq): parity.check_float allows every bin
2e-6 of the row's largest bin.  On synth_iq, the recorded captures and the constant and square-wave frames that bin is
the offset-binary DC term or a tone, a hundred to a thousand times above the rest, so a fault that turns some bins by
2e-5 rad -- a table entry a twentieth of an index step off at 16384 points, a contraction the compiler introduces --
passes every value test of the suite.  On a frame whose reference has no dominant bin (crest condition: max <= 4 median)
the same bound, unchanged, refuses it.  tests/test_gpu_flat.py runs these families on the device.

Frame subsets of the emulator tests (the tier's time): the default configuration of a size sees every position of
flat_ref.positions(n) in mode 3 with raw int8 bytes; every other combination (offset-binary bytes, pair frames in the
other modes, f32 input, shift, tapers) every 4th position and the last one, every tuning variant every 8th and the last.
The first positions of positions(n) at 2048 points and above are 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, ...: a stride keeps
every power of two times some odd digit, not every digit at every stride; that is the full set's job."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_ref as F
from tests import parity
from tests.conftest import synth_iq
from tests.emu_util import emu_rows
from tests.test_emu_kernels import SIZES

SHIFTS = ((-0.123456789, 0.75), (0.4999, 0.75))


def every(pos, step):
    pos = np.asarray(pos)
    return np.unique(np.r_[pos[::step], pos[-1]])


# ---- the families are what they claim ----

@pytest.mark.parametrize("n", SIZES)
def test_closed_form_equals_the_oracle(n):
    """X[k] = sum a (-1)^p e^{-2 pi i p k / n} against O.rows(..., MODE_COMPLEX): every position up to 1024 points, 16 at
    each larger size; both byte conventions; single impulses, pairs, sparse frames, shifted frames (all bins but n/2,
    where the shifter's 0.5 (1 + i) lands whole: asserted too)."""
    pos = F.positions(n) if n <= 1024 else every(F.positions(n), len(F.positions(n)) // 15)
    for flip in (True, False):
        for iq, pl in (F.impulse_frames(n, flip, pos), F.pair_frames(n, flip, pos), F.sparse_frames(n, 4, 8, 1, flip)):
            want = O.rows(iq.ravel(), len(pl), n, flip=flip, mode=O.MODE_COMPLEX)
            assert np.abs(F.spectra(n, pl) - want).max() <= 1e-12
    pos = every(pos, max(1, len(pos) // 15))
    for kind in (F.impulse_frames, F.pair_frames):
        iq, pl = kind(n, True, pos)
        want = O.rows_shifted(iq.ravel(), len(pl), n, *SHIFTS[0], mode=O.MODE_COMPLEX)
        closed = F.spectra(n, pl, shift=SHIFTS[0])
        assert np.abs((closed - want)[:, F.not_dc(n)]).max() <= 1e-12
        assert np.abs((want - closed)[:, n // 2] - 0.5 * n * (1 + 1j)).max() <= 1e-9 * n


@pytest.mark.parametrize("n", SIZES + [3, 31, 1000, 1001, 8193, 1 << 15, 1 << 16, 1 << 17])
def test_crest_condition_holds_for_every_family(n):
    """max |want| <= 4 median |want| over the compared bins, for every frame the two test files use: a condition on the
    inputs.  Closed forms (held to the oracle above) where the whole position set is large."""
    power_of_two_kernel = n in SIZES
    if not power_of_two_kernel:         # the any-size families: f32 impulses and noise
        pos = F.any_size_positions(n)
        assert n - 1 in pos and pos.max() < n and len(pos) <= 32
        assert F.crest(F.impulses_f64(n, pos[:8])[1]) <= 1.0 + 1e-9
        assert F.crest(F.noise_f64(n, 3, 5)[1]) <= F.CREST_MAX
        return
    pos = F.positions(n)
    assert F.crest(F.spectra(n, F.impulse_placements(pos))) <= 1.0 + 1e-9
    assert F.crest(F.spectra(n, F.pair_placements(pos))) <= 3.0 + 1e-9
    assert F.crest(np.abs(F.spectra(n, F.pair_placements(pos)))) <= F.CREST_MAX
    assert F.crest(F.spectra(n, F.sparse_frames(n, 8, 8, 1)[1])) <= F.CREST_MAX
    assert F.crest(F.noise_f64(n, 8, 3)[1]) <= F.CREST_MAX
    keep = F.not_dc(n)
    for shift in SHIFTS:
        assert F.crest(F.spectra(n, F.impulse_placements(pos), shift=shift), keep) <= 1.0 + 1e-9
        assert F.crest(F.spectra(n, F.pair_placements(pos), shift=shift), keep) <= 3.0 + 1e-9
    for wname in ("hann", "random"):
        for kind in ("impulse", "pair"):
            iq, pl, want, keep, w = F.windowed_case(n, wname, kind, pos=every(pos, 4))
            assert len(pl) >= 4
            assert F.crest(want, keep) <= (1.001 if kind == "impulse" else 3.001)      # (the floor on the inner ring)
    iq, pl, want, keep, w = F.windowed_case(n, "hann", "impulse", pos=every(pos, 8), shift=SHIFTS[0])
    assert F.crest(want, keep) <= 1.001
    if n >= 8192:
        stream, pl = F.half_overlap_stream(n, 9)
        want = O.rows(stream, 9, n, hop=n // 2, mode=O.MODE_COMPLEX)
        assert np.abs(F.spectra(n, pl) - want).max() <= 1e-12
        assert F.crest(want) <= 3.0 + 1e-9


@pytest.mark.parametrize("n", SIZES)
def test_band_condition_of_the_centred_form(n):
    """Frames for the centred form of the windowed kernels (0x80 background, Hann rounded to f32): on the outer ring of
    flat_ref.centred_rings, what the reference (oracle's rows less the background's row) holds beside the impulse is
    below 1e-9 of the impulse.  The background's own row is NOT that small outside the BAND bins round n/2 -- the f32
    rounding of the weights spreads its 0.5 (1 + i) over every bin, up to 1e-4 of the smallest impulse (printed) -- which
    is why it is taken off where the kernels leave it out: it stays inside the criterion under which
    build_window_tables picks the centred form, an rms of 2^-24 sqrt(0.5 sum w^2)."""
    iq, pl, want, keep, w = F.windowed_case(n, "hann", "impulse")
    w64 = w.astype(np.float64)
    closed = F.spectra(n, pl, 0x80, w64)
    size = np.abs(closed).min(axis=1, keepdims=True)
    assert size.min() >= 0.1 * abs(F.amplitude(F.SINGLE[0x80], 0x80)) * 0.999
    inner, outer = F.centred_rings(n)
    assert np.array_equal(keep, inner | outer) and outer.sum() >= n // 2 - 2 and not (inner | outer)[n // 2 - F.BAND: n // 2 + F.BAND + 1].any()
    assert np.max(np.abs((want - closed)[:, outer]) / size) <= 1e-9
    background = O.rows_windowed(F.build_frames(n, [[]], 0x80, True).ravel(), 1, n, w64, mode=O.MODE_COMPLEX)[0]
    if inner.any():                                                      # there the reference keeps the floor, and nothing else
        assert np.max(np.abs((want - closed - background)[:, inner]) / size) <= 1e-9
    keep = F.band_keep(n)
    floor = np.abs(background[keep])
    print("n=%d: background outside the band max %.2e rms %.2e, smallest impulse %.3f" % (
        n, floor.max(), np.sqrt(np.mean(floor ** 2)), size.min()))
    assert np.sqrt(np.mean(floor ** 2)) <= 2.0 ** -24 * np.sqrt(0.5 * np.sum(w64 ** 2))
    inside = np.abs(background[~keep])
    assert inside.max() >= 0.2 * n                                       # the DC term itself: inside the band


@pytest.mark.parametrize("n", SIZES)
def test_positions_cover_every_digit_at_every_stride(n):
    """For every radix R = 2 ... 32 and every power-of-two stride s with R s <= n, every digit value r = 1 ... R - 1
    occurs as the position r s: a single nonzero digit whatever the radix order."""
    pos = set(int(p) for p in F.positions(n))
    assert n - 1 in pos and max(pos) < n and min(pos) >= 0
    if n > 1024:
        assert 100 <= len(pos) <= 270
    for radix in (2, 4, 8, 16, 32):
        s = 1
        while radix * s <= n:
            missing = [r * s for r in range(1, radix) if r * s not in pos]
            assert not missing, (radix, s, missing)
            s *= 2


# ---- the kernel source on the same families (tests/emu) ----

@pytest.mark.parametrize("n", SIZES)
def test_emu_impulses_complex(n):
    pos = F.positions(n)
    iq, pl = F.impulse_frames(n, True, pos)
    got = emu_rows(iq.ravel(), n, len(pl), mode=3, specialised=False)
    worst = F.check_rows(parity.check_float, got, F.spectra(n, pl), "emu n=%d u8" % n, F.labels(pl))
    iq, pl = F.impulse_frames(n, False, every(pos, 4))
    got = emu_rows(iq.ravel(), n, len(pl), flip=False, mode=3, specialised=False, grid=3)
    F.check_rows(parity.check_float, got, F.spectra(n, pl), "emu n=%d u8 offset binary" % n, F.labels(pl))
    iq, pl = F.sparse_frames(n, 8, 8, 1)
    got = emu_rows(iq.ravel(), n, len(pl), mode=3, specialised=False)
    F.check_rows(parity.check_float, got, F.spectra(n, pl), "emu n=%d sparse" % n, F.labels(pl))
    print("emulator, n=%d: worst per-bin relative error on single impulses %.2e" % (n, worst))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", [0, 1, 2, 4, 5])
def test_emu_pairs_other_modes(n, mode):
    iq, pl = F.pair_frames(n, True, every(F.positions(n), 4))
    got = emu_rows(iq.ravel(), n, len(pl), mode=mode, specialised=mode in (0, 1, 2))
    F.check_mode_rows(got, F.spectra(n, pl), mode, "emu n=%d pairs" % n, F.labels(pl))


@pytest.mark.parametrize("n", SIZES)
def test_emu_f32_input(n):
    x, spec = F.noise_f64(n, 4, 7)
    for mode in (0, 3):
        got = emu_rows(x.astype(np.float32), n, 4, mode=mode, in_kind=1, specialised=False)
        F.check_mode_rows(got, spec, mode, "emu n=%d f32 noise" % n, ["noise frame"] * 4)
    pos = every(F.positions(n), 4)
    x, spec = F.impulses_f64(n, pos)
    got = emu_rows(x.astype(np.float32), n, len(pos), mode=3, in_kind=1, specialised=False)
    F.check_rows(parity.check_float, got, spec, "emu n=%d f32 impulses" % n, ["impulse at %d" % p for p in pos])


@pytest.mark.parametrize("n", [s for s in SIZES if s >= 128])
def test_emu_shifted(n):
    keep = F.not_dc(n)
    pos = every(F.positions(n), 4)
    for (kind, mode), shift in zip(((F.impulse_frames, 3), (F.pair_frames, 0)), SHIFTS):
        iq, pl = kind(n, True, pos)
        got = emu_rows(iq.ravel(), n, len(pl), mode=mode, grid=2, shift=shift)
        want = O.rows_shifted(iq.ravel(), len(pl), n, shift[0], shift[1], mode=O.MODE_COMPLEX)
        F.check_mode_rows(got, want, mode, "emu n=%d shifted by %r" % (n, shift[0]), F.labels(pl), keep)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("wname", ["hann", "random"])
@pytest.mark.parametrize("wmode", [1, 2])
def test_emu_windowed(n, wname, wmode):
    for kind, mode in (("impulse", 3), ("pair", 0)):
        iq, pl, want, keep, w = F.windowed_case(n, wname, kind, pos=every(F.positions(n), 4))
        got = emu_rows(iq.ravel(), n, len(pl), mode=mode, window=w, window_mode=wmode, specialised=mode == 0)
        if mode == 0 and keep is None:
            keep = F.not_dc(n)          # |X| on every bin but the patched one
        F.check_mode_rows(got, want, mode, "emu n=%d %s taper, WIN %d" % (n, wname, wmode), F.labels(pl), keep)


VARIANTS = [(8192, "nd"), (8192, "v2"), (8192, "v2s"), (8192, "x0"), (8192, "A"), (8192, "B"), (8192, "D"), (8192, "B2"),
            (8192, "D2"), (8192, "W"), (8192, "notwl"), (8192, "notwr"), (4096, "nr"), (2048, "nr"), (4096, "x0"), (4096, "df"),
            (4096, "t256"), (4096, "B3"), (4096, "B"), (4096, "C"), (4096, "D"), (2048, "x0"), (2048, "df"), (2048, "B"),
            (2048, "C"), (1024, "x0"), (1024, "B"), (1024, "C"), (1024, "D"), (16384, "nd"), (16384, "B"), (256, "p16"),
            (128, "p16"), (4096, "w64"), (4096, "w64b"), (4096, "s2"), (4096, "pk"), (4096, "px0"), (8192, "pk"), (8192, "px0"),
            (256, "pk"), (256, "px0"), (1024, "px0"), (256, "p64"), (1024, "r2"), (1024, "e"), (1024, "h"),
            (256, "rows"), (512, "px"), (1024, "rt")]


@pytest.mark.parametrize("n,variant", VARIANTS)
def test_emu_tuning_variants(n, variant):
    """The list of test_emu_kernels.py::test_tuning_variants (w64 and w64b are in it) and the three per-mode product
    configurations."""
    pos = every(F.positions(n), 8)
    iq, pl = F.impulse_frames(n, True, pos)
    got = emu_rows(iq.ravel(), n, len(pl), mode=3, specialised=False, variant=variant)
    F.check_rows(parity.check_float, got, F.spectra(n, pl), "emu n=%d variant %s" % (n, variant), F.labels(pl))
    iq, pl = F.pair_frames(n, True, pos)
    got = emu_rows(iq.ravel(), n, len(pl), mode=0, variant=variant)
    F.check_mode_rows(got, F.spectra(n, pl), 0, "emu n=%d variant %s pairs" % (n, variant), F.labels(pl))


@pytest.mark.parametrize("n", [8192, 16384])
def test_emu_half_overlap(n):
    nf = 9
    stream, pl = F.half_overlap_stream(n, nf)
    got = emu_rows(stream, n, nf, hop=n // 2, grid=2, run_len=4)
    F.check_mode_rows(got, F.spectra(n, pl), 0, "emu n=%d half overlap" % n, F.labels(pl))
    assert np.array_equal(got, emu_rows(stream, n, nf, hop=n // 2, grid=2, dynamic_units=False))


# ---- the comparison's teeth ----

def test_a_small_turn_fails_on_flat_frames_and_passes_on_synth_iq():
    """Reference against reference, no wrong build: the bins of one residue class mod 8 turned by 2e-5 rad -- what one
    twiddle-table entry that far off does.  On an impulse frame check_float refuses it (per bin 2.5e-5 against an
    allowance of 3.5e-6, relative L2 7e-6 against 1e-6); the same turn of a synth_iq frame's reference at 8192 points
    stays a twentieth of its per-bin allowance, because 2e-6 of that row's DC term is 1.2e-2 and an ordinary bin is 10,
    and with half as many bins turned (a class mod 16) passes check_float whole.  MAG rows need the pair: a turned
    single impulse has the magnitudes it had, the weak impulse of a pair turned against the strong one has not."""
    n = 8192
    iq, pl = F.impulse_frames(n, True, [1234])
    want = F.spectra(n, pl)[0]
    parity.check_float(want.astype(np.complex64), want)
    with pytest.raises(AssertionError):
        parity.check_float(F.turn_residue_class(want).astype(np.complex64), want)
    with pytest.raises(AssertionError):
        parity.check_float(F.turn_residue_class(want, modulus=16).astype(np.complex64), want)
    ordinary = O.rows(synth_iq(n, 2 * n), 1, n, mode=O.MODE_COMPLEX)[0]
    assert F.crest(ordinary) > 100.0
    # per bin the turn of the whole class mod 8 is a twentieth of the allowance; in L2 a full eighth of the bins comes to
    # 1.07e-6, a hair over the 1e-6 (905 / sqrt(8) * 2e-5 over a norm of 6000): a class mod 16 -- a table entry feeds
    # fewer bins still -- passes whole, and fails above on the flat frame
    turned = F.turn_residue_class(ordinary)
    assert np.abs(turned - ordinary).max() <= (parity.PER_BIN_TOL * np.abs(ordinary).max() + 1e-6) / 20.0
    assert np.linalg.norm(turned - ordinary) / np.linalg.norm(ordinary) <= 1.1e-6
    rel, worst = parity.check_float(F.turn_residue_class(ordinary, modulus=16).astype(np.complex64), ordinary)
    assert worst > 1e-5 * np.median(np.abs(ordinary))
    parity.check_float(np.abs(F.turn_residue_class(want)).astype(np.float32), np.abs(want))     # a single impulse in MAG: blind
    (strong, weak), = F.pair_placements([1234])
    s, w = F.spectra(n, [[strong]])[0], F.spectra(n, [[weak]])[0]
    parity.check_float(np.abs(s + w).astype(np.float32), np.abs(s + w))
    with pytest.raises(AssertionError):
        parity.check_float(np.abs(s + F.turn_residue_class(w)).astype(np.float32), np.abs(s + w))
    want_db = parity.rows_of_spectra((s + w)[None], 5)[0]
    parity.check_db_bins(want_db.astype(np.float32), want_db, np.abs(s + w))
    with pytest.raises(AssertionError):
        parity.check_db_bins(parity.rows_of_spectra((s + F.turn_residue_class(w))[None], 5)[0], want_db, np.abs(s + w))
