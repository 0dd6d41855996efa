"""GPU tier (-m gpu): every FFT path on inputs whose reference row has no dominant bin (tests/flat_ref.py), so that
parity.check_float's per-bin allowance -- 2e-6 of the row's largest bin -- is 2e-6 of EVERY bin.  On synth_iq and the
recorded captures it is 1e-3 of an ordinary bin, and a few bins turned by 1e-5 ... 1e-3 of their size pass
(tests/test_flat_host.py shows both, reference against reference).  Nothing here has a bound of its own: single impulses,
pairs, sparse frames and zero-mean noise go frame by frame (one call per frame: the max is that frame's) through
check_float, check_u8 and, for dB rows, parity.check_db_bins as they stand.  A failure names size, path, impulse
positions and the worst bin; every test prints the worst per-bin relative error it saw ("FLAT ..." lines: figures for
DESIGN.md section 6, no bounds).

References: the closed form of flat_ref.spectra for the un-windowed u8 frames (held to the oracle's rows on the CPU tier),
the oracle's own rows for the shifted, windowed and f64 paths, any_size_spectra's long-double DFT / numpy's f64 FFT for the
sizes without a kernel.  The shifter's 0.5 (1 + i) lands in bin n/2, which shifted rows leave out; the centred form of the
windowed kernels is compared on flat_ref.centred_rings.

Not here: u8 input on the any-size paths.  They transform (u - 128) / 256 in f32 and add the offset's spectrum afterwards
("Where 'same tolerance' needs a qualification"): over a zero background that is a cancellation of two
parts a thousand times the impulse, and a flat comparison would need a widened rule.  Their arithmetic is reached through
f32 input instead.  The open four-step case (2^18 points, hop n/2) stays out as well."""
import functools

import numpy as np
import pytest

from frequensea_amd import fsea
from oracle import oracle as O
from tests import flat_ref as F
from tests import parity
from tests.conftest import kernel_stem

pytestmark = pytest.mark.gpu

SIZES = [32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]
POLICY = {"auto": fsea.UNITS_AUTO, "tickets": fsea.UNITS_TICKETS, "static": fsea.UNITS_STATIC}
# the multi-wave sizes under both unit distributions: a launch of 260 frames reaches the ticket pools only when pinned
PLAN_CASES = [(n, "auto") for n in SIZES if n < 4096] + [(n, p) for n in SIZES if n >= 4096 for p in ("tickets", "static")]
SHIFTS = ((-0.123456789, 0.75), (0.4999, 0.75))


def make_plan(n, mode, policy="auto", hop=None):
    plan = fsea.Plan(n, hop=hop, mode=mode)
    plan.set_unit_distribution(POLICY[policy])
    return plan


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=2)
def impulse_case(n):
    """(raw int8 bytes, offset-binary bytes, placements, closed-form spectra) of the single-impulse frames; read-only."""
    iq, pl = F.impulse_frames(n, True)
    return frozen(iq, iq ^ np.uint8(0x80), pl, F.spectra(n, pl))


@functools.lru_cache(maxsize=2)
def pair_case(n):
    iq, pl = F.pair_frames(n, True)
    return frozen(iq, iq ^ np.uint8(0x80), pl, F.spectra(n, pl))


def report(what, figure):
    print("FLAT %s: %.3e" % (what, figure))


@pytest.mark.parametrize("n,policy", PLAN_CASES)
def test_single_impulses_complex_rows(n, policy):
    """One impulse per frame at every position of flat_ref.positions(n), mode 3, both byte conventions: every bin of the
    reference has the same size.  Eight sparse frames of eight random impulses ride along."""
    raw, off, pl, spec = impulse_case(n)
    plan = make_plan(n, 3, policy)
    assert plan.kernel_name.startswith(kernel_stem(n, 3))
    worst = 0.0
    for flip, iq in ((True, raw), (False, off)):
        got = plan.exec_host(iq.ravel(), len(pl), flip=flip)
        worst = max(worst, F.check_rows(parity.check_float, got, spec, "n=%d u8 flip=%s %s" % (n, flip, policy), F.labels(pl)))
    iq, spl = F.sparse_frames(n, 8, 8, 1)
    got = plan.exec_host(iq.ravel(), len(spl))
    F.check_rows(parity.check_float, got, F.spectra(n, spl), "n=%d u8 sparse %s" % (n, policy), F.labels(spl))
    plan.close()
    report("n=%d u8 complex %s, worst per-bin relative error" % (n, policy), worst)


@pytest.mark.parametrize("mode", [0, 1, 2, 4, 5])
@pytest.mark.parametrize("n,policy", PLAN_CASES)
def test_pairs_in_every_other_mode(n, policy, mode):
    """A weak impulse beside a fixed one of twice its size: the phase of every bin shows in its magnitude, so MAG, MAG_NODC,
    dB and pixel rows see a turned bin.  Every mode takes its own configuration of the size where it has one (256 points
    "rows", 512 "px", 1024 "rt": conftest.kernel_stem); raw int8 bytes run the compile-time kernels of modes 0, 1 and 2,
    offset-binary bytes the run-time-mode kernel."""
    raw, off, pl, spec = pair_case(n)
    plan = make_plan(n, mode, policy)
    assert plan.kernel_name.startswith(kernel_stem(n, mode))
    figure = -np.inf
    for flip, iq in ((True, raw), (False, off)):
        got = plan.exec_host(iq.ravel(), len(pl), flip=flip)
        figure = max(figure, F.check_mode_rows(got, spec, mode, "n=%d u8 pairs flip=%s %s" % (n, flip, policy), F.labels(pl)))
    plan.close()
    report("n=%d u8 pairs mode %d %s, %s" % (n, mode, policy, {1: "pixels one level off", 2: "pixels one level off",
                                                                 5: "worst excess over the allowance through the log, dB"}.get(
                                                                     mode, "worst per-bin relative error")), figure)


@pytest.mark.parametrize("n,mode", [(256, 0), (512, 1), (1024, 3)])
def test_first_configuration_of_the_sizes_with_two(n, mode, monkeypatch):
    """FSEA_ONE_CONFIG_PER_SIZE=1 at plan creation: the size's first configuration in a mode that would take another."""
    monkeypatch.setenv("FSEA_ONE_CONFIG_PER_SIZE", "1")
    raw, off, pl, spec = impulse_case(n) if mode == 3 else pair_case(n)
    plan = fsea.Plan(n, mode=mode)
    assert plan.kernel_name.startswith("fsea_fft%d_" % n)
    got = plan.exec_host(raw.ravel(), len(pl))
    plan.close()
    F.check_mode_rows(got, spec, mode, "n=%d first configuration" % n, F.labels(pl))


@pytest.mark.parametrize("n", SIZES)
def test_f64_input_noise_and_impulses(n):
    """exec_host_f64: zero-mean noise (sigma 0.2, frames inside the crest condition) in modes 0 and 3 against the oracle's
    FFT, and impulses on exact zeros in mode 3 against the closed form."""
    nf = 8
    x, _ = F.noise_f64(n, nf, 11)
    spec = np.stack([O.fft_forward(O.unpack_center_f64(x[f])) for f in range(nf)])
    noise = worst = 0.0
    for mode in (0, 3):
        plan = fsea.Plan(n, mode=mode)
        got = plan.exec_host_f64(x.ravel(), nf)
        noise = max(noise, F.check_mode_rows(got, spec, mode, "n=%d f64 noise" % n, ["noise frame %d" % f for f in range(nf)], per="median"))
        if mode == 3:
            pos = F.positions(n)
            xi, si = F.impulses_f64(n, pos)
            got = plan.exec_host_f64(xi.ravel(), len(pos))
            worst = F.check_rows(parity.check_float, got, si, "n=%d f64 impulses" % n, ["impulse at %d" % p for p in pos])
        plan.close()
    report("n=%d f64 impulses, worst per-bin relative error" % n, worst)
    report("n=%d f64 noise, worst per-bin error over the row's median" % n, noise)


@pytest.mark.parametrize("n", [s for s in SIZES if s >= 128])
def test_frequency_shifted_impulses_and_pairs(n):
    """exec_shifted_host at -0.123456789 and 0.4999 cycles per sample, phase 0.75: impulses in mode 3, pairs in mode 0,
    against the oracle's shifter and F64-branch FFT on every bin but n/2."""
    keep = F.not_dc(n)
    worst = 0.0
    for shift in SHIFTS:
        for (raw, off, pl, spec), mode in ((impulse_case(n), 3), (pair_case(n), 0)):
            plan = fsea.Plan(n, mode=mode)
            got = plan.exec_shifted_host(raw.ravel(), len(pl), shift[0], shift[1])
            plan.close()
            want = O.rows_shifted(raw.ravel(), len(pl), n, shift[0], shift[1], mode=O.MODE_COMPLEX)
            worst = max(worst, F.check_mode_rows(got, want, mode, "n=%d shifted by %r" % (n, shift[0]), F.labels(pl), keep))
    report("n=%d u8 shifted, worst per-bin relative error" % n, worst)


@pytest.mark.parametrize("n", [1024, 8192])
def test_frequency_shifted_pairs_at_half_hop(n):
    nf, hop = 65, n // 2
    stream, pl = F.half_overlap_stream(n, nf)
    keep = F.not_dc(n)
    for shift, mode in zip(SHIFTS, (3, 0)):
        plan = fsea.Plan(n, hop=hop, mode=mode)
        got = plan.exec_shifted_host(stream, nf, shift[0], shift[1])
        plan.close()
        want = O.rows_shifted(stream, nf, n, shift[0], shift[1], hop=hop, mode=O.MODE_COMPLEX)
        F.check_mode_rows(got, want, mode, "n=%d hop n/2 shifted by %r" % (n, shift[0]), F.labels(pl), keep)


@pytest.mark.parametrize("wname", ["hann", "random"])
@pytest.mark.parametrize("n", SIZES)
def test_windowed_impulses_and_pairs(n, wname):
    """A taper on the plan: "hann" runs the centred form (0x80 background, the oracle's rows less the background's where
    the kernels leave its floor out: flat_ref.centred_rings), "random" the offset-binary form (zero background, the
    oracle's rows).  Impulses where |w| >= 0.1 in mode 3; pairs in mode 0, the fixed impulse where |w| is largest."""
    worst = 0.0
    for kind, mode in (("impulse", 3), ("pair", 0)):
        iq, pl, want, keep, w = F.windowed_case(n, wname, kind)
        plan = fsea.Plan(n, mode=mode)
        plan.set_window(w)
        assert plan.window_form == (2 if wname == "random" else 1)
        got = plan.exec_host(iq.ravel(), len(pl))
        plan.close()
        if mode == 0 and keep is None:
            keep = F.not_dc(n)
        worst = max(worst, F.check_mode_rows(got, want, mode, "n=%d %s taper" % (n, wname), F.labels(pl), keep))
    report("n=%d u8 %s taper, worst per-bin relative error" % (n, wname), worst)


@pytest.mark.parametrize("n", [1024, 8192])
def test_windowed_shifted_and_windowed_f64(n):
    iq, pl, want, keep, w = F.windowed_case(n, "hann", "impulse", shift=SHIFTS[0])
    plan = fsea.Plan(n, mode=3)
    plan.set_window(w)
    got = plan.exec_shifted_host(iq.ravel(), len(pl), *SHIFTS[0])
    worst = F.check_mode_rows(got, want, 3, "n=%d hann taper, shifted" % n, F.labels(pl), keep)
    pos = F.window_positions(n, w)
    x, _ = F.impulses_f64(n, pos)
    want = O.rows_f64(x.ravel(), len(pos), n, mode=O.MODE_COMPLEX, window=w.astype(np.float64))
    assert F.crest(want) <= 1.0 + 1e-9
    got = plan.exec_host_f64(x.ravel(), len(pos))
    plan.close()
    worst = max(worst, F.check_rows(parity.check_float, got, want, "n=%d hann taper, f64" % n, ["impulse at %d" % p for p in pos]))
    report("n=%d hann taper shifted / f64, worst per-bin relative error" % n, worst)


@pytest.mark.parametrize("n", [8192, 16384])
def test_half_overlap_kernel_on_pair_frames(n, monkeypatch):
    """`*_u8_mag_half` (hop n/2): a stream in which every frame is a pair frame and consecutive frames share half a frame,
    against the oracle, and bit for bit against the ordinary kernel (FSEA_NO_HALF_OVERLAP=1 at plan creation)."""
    nf, hop = 257, n // 2
    stream, pl = F.half_overlap_stream(n, nf)
    rows = {}
    for half in (True, False):
        if half:
            monkeypatch.delenv("FSEA_NO_HALF_OVERLAP", raising=False)
        else:
            monkeypatch.setenv("FSEA_NO_HALF_OVERLAP", "1")
        plan = fsea.Plan(n, hop=hop)
        assert plan.kernel_name == "fsea_fft%d_u8_mag%s" % (n, "_half" if half else "")
        rows[half] = plan.exec_host(stream, nf)
        plan.close()
    assert np.array_equal(rows[True], rows[False])
    want = O.rows(stream, nf, n, hop=hop, mode=O.MODE_COMPLEX)
    assert F.crest(want) <= 3.0 + 1e-9
    report("n=%d half overlap, worst per-bin relative error" % n,
           F.check_mode_rows(rows[True], want, 0, "n=%d half-overlap kernel" % n, F.labels(pl)))


@pytest.mark.parametrize("n", [3, 31, 1000, 1001, 8193, 1 << 15, 1 << 16, 1 << 17])
def test_any_size_paths_on_f32_input(n):
    """Bluestein (3, 31, 1000, 1001, 8193 points) and four-step (2^15 = 256 x 128, 2^16 = 256 x 256, 2^17 = 512 x 256:
    fourstep_split gives a size one split, so the unequal and the equal one are two sizes) in mode 3 on float input, which
    exec_host_f64 narrows and leaves resident on the device: zero-mean noise and impulses on exact zeros
    (flat_ref.any_size_positions: strides and positions with both four-step digits nonzero).  Reference: the oracle's
    long-double DFT up to 1001 points, numpy's f64 FFT above, for the noise; the closed form for the impulses."""
    nf = 3
    x, spec = F.noise_f64(n, nf, 13)
    if n <= 1001:
        spec = np.stack([O.dft_naive(F.centred(x[f])) for f in range(nf)])
    plan = fsea.Plan(n, mode=3)
    path = plan.kernel_name.split("(")[0]
    assert path in ("bluestein", "fourstep")
    got = plan.exec_host_f64(x.ravel(), nf)
    noise = F.check_rows(parity.check_float, got, spec, "n=%d f32 noise" % n, ["noise frame %d" % f for f in range(nf)], per="median")
    pos = F.any_size_positions(n)
    xi, si = F.impulses_f64(n, pos)
    got = plan.exec_host_f64(xi.ravel(), len(pos))
    plan.close()
    worst = F.check_rows(parity.check_float, got, si, "n=%d f32 impulses" % n, ["impulse at %d" % p for p in pos])
    report("n=%d any-size f32 impulses (%s), worst per-bin relative error" % (n, path), worst)
    report("n=%d any-size f32 noise (%s), worst per-bin error over the row's median" % (n, path), noise)
