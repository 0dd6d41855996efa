"""GPU tier: the shifted paths over the argument domain they document -- stream positions up to 2^52 (across 2^24, 2^31,
2^32 and 2^40), |cycles_per_sample| up to 2^20 (0.5, 1.0, tiny, subnormal and -0.0 among them), any finite phase0_cycles --
for fsea_fir_u8_shifted_host / _device, fsea_chain_run_host / _device, fsea_zoom_run_host / _device and the host blocks
nrf_iq_chain and nrf_zoom_fft at a `consumed` of 2^44.

Against tests/shift_ref.py (the phase in exact rational arithmetic, rounded once) through check of tests/test_gpu_fir.py
with its MAX_ABS and MAX_REL as they stand: their derivation holds at every position because the kernel's phase reduction
stays within 2^-30 cycles of the exact phase over the whole domain (tests/test_shift_ref_host.py), 1/32 of what the float
conversion behind it adds.  Taps: lowpass_like_taps of tests/test_gpu_zoom.py (S = 1, DC gain 1: the premises of those
bounds).  Bit for bit: host form == device form, zoom pairs == every D-th output of the filter, rows == the plan's rows on
the pairs, a stream cut into calls == one call.  Device outputs are Guarded payloads (tests/guarded.py); inputs stand
between two fills once, above 2^32.  A refused chain call changes nothing.

The shapes are the smallest that reach every path of the staging: n in {1, 7, 9, 2 * 2048 + 13} (a tile is 2048 outputs),
L in {21, 512}, D in {3, 16} with n = D (2 * 128 + 5) + 1."""
import ctypes

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import shift_ref
from tests.guarded import FILL, Guarded
from tests.test_gpu_bounds import INPUT_FILLS, Outputs, fenced, same
from tests.test_gpu_fir import MAX_ABS, check, u8_to_complex
from tests.test_gpu_zoom import lowpass_like_taps
from tests.test_fir_host import fir_reference
from tests.test_shift_ref_host import BAD_SHIFTS, GRID_CYCLES, GRID_N, GRID_PHASES, LIMIT, grid_positions

pytestmark = pytest.mark.gpu

FSEA_EINVAL = -1
CPS, PHASE0 = -1.2e6 / 10e6, 0.75
EVERYWHERE = [(c, p) for c in (CPS, 1048575.999, 0.4999) for p in (0.75, -12345.678)]    # at every position
ABOVE = 1 << 40                                 # the position of the residues and the fences
ZT = fsea.ZOOM_TILE_OUTPUTS
CUT_START, CUT_N = (1 << 32) - 4100, 8192       # the cut streams: 2^32 inside, no multiple of 8 at the start


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def combos(n, residues=False):
    """(sample_offset, cycles_per_sample, phase0_cycles) of a call of n samples: every position with three cycles and two
    phases; every cycle with every phase at two positions, across 2^31 and at the last admissible call; with `residues`
    all eight sample_offset mod 8 above 2^32 (stage_group's two-base path is taken for seven of them)."""
    pos = grid_positions(n)
    out = [(p, c, ph) for p in pos for c, ph in EVERYWHERE]
    out += [(p, c, ph) for p in (pos[2], pos[5]) for c in GRID_CYCLES for ph in GRID_PHASES]
    if residues:
        out += [(ABOVE + r, CPS, PHASE0) for r in range(8)]
    return out


def test_the_grid_is_the_one_the_host_tier_holds_the_reduction_on():
    pos = grid_positions(GRID_N)
    assert pos[3] < (1 << 32) < pos[3] + GRID_N and ((1 << 32) - pos[3]) % 2048 not in (0, 2047)   # inside a tile
    assert pos[5] + GRID_N == LIMIT and len(GRID_CYCLES) == 12 and len(GRID_PHASES) == 5
    assert {p & 7 for p, _, _ in combos(9, True)} == set(range(8))


# ---- the filter -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("L", [21, 512])
def test_fir_host_and_device_forms_against_the_exact_reference(L, flip):
    """The long call runs on a fresh tail.  A short call (n = 1, 7, 9) on a fresh tail is a few taps times a few samples,
    y ~ 1e-4 at L = 512: the premise of MAX_REL, rms(y) >= ~0.3, does not hold for it (one such output, rotated part and
    0.5 nearly cancelling, measured 3e-6 relative at 5.6e-10 absolute).  So a short call stands between a call of L - 1
    samples that fills the tail and one of 9 samples that reads the tail the short call wrote (the copy of the old tail
    for n < L - 1 among it).  The outputs of the three calls together are held to both bounds: MAX_ABS is a bound on every
    output, MAX_REL one on a signal of many outputs whose errors average (tests/test_gpu_fir.py derives it from
    independent errors; one standard deviation of a single output is sqrt(L / 3) u 1.5 = 1.2e-6 at L = 512).  A short
    call held to MAX_REL alone is a single output held to it: at L = 512, n = 1, position 2^32 - 2053 one such output,
    |y| = 0.33, came back 4.9e-7 off (MAX_ABS / 20), 1.49e-6 relative -- the f32 accumulation of 512 taps, not the shift.
    The short call stands at the grid position, the other two just below it: a call's position is its own argument."""
    c = lowpass_like_taps(L, L)
    fir = fsea.Fir(c)
    rng = np.random.default_rng(10 * L + flip)
    for n in (1, 7, 9, GRID_N):
        lengths = [n] if n == GRID_N else [L - 1, n, 9]
        data = [rng.integers(0, 256, 2 * k, dtype=np.uint8) for k in lengths]
        d_ins = [fsea.DeviceBuffer(max(2 * k, 16)).upload(iq) for k, iq in zip(lengths, data)]
        outs = [Guarded(8 * k) for k in lengths]
        for offset, cps, ph in combos(n, residues=n == 9):
            what = (L, flip, n, offset, cps, ph)
            at = [offset] if n == GRID_N else [max(offset - (L - 1), 0), offset, max(offset - 9, 0)]
            fir.reset()
            host, wants, tail = [], [], None
            for iq, pos in zip(data, at):
                want, tail = shift_ref.shifted_fir_reference(iq, flip, cps, ph, c, tail, offset=pos)
                host.append(fir.run_u8_shifted(iq, cps, ph, pos, flip=bool(flip)))
                wants.append(want)
            check(np.concatenate(host), np.concatenate(wants), ("host",) + what)
            fir.reset()
            for k, d_in, out, pos, got in zip(lengths, d_ins, outs, at, host):
                out.upload(np.full(8 * k, FILL, np.uint8))
                fir.run_shifted_device(d_in.ptr.value, k, out.addr, cps, ph, pos, flip=bool(flip))
                out.check(what)
                assert np.array_equal(bits(out.payload(np.complex64, k)), bits(got)), what + (k,)
        for b in d_ins + outs:
            b.free()
    fir.close()


def seeded_cuts(total, L, seed, multiple=1):
    """Call lengths that sum to `total`: 1, lengths below L - 1 and random ones, all multiples of `multiple` but the last."""
    rng = np.random.default_rng(seed)
    cuts = [1, max(L - 2, 1), 3, 1, L // 2 + 1] if multiple == 1 else [multiple, 2 * multiple]
    while sum(cuts) < total - 1500:
        cuts.append(int(rng.integers(1, 1500 // multiple + 1)) * multiple)
    cuts.append(total - sum(cuts))
    assert cuts[-1] > 0 and sum(cuts) == total
    return cuts


@pytest.mark.parametrize("L", [21, 512])
def test_fir_stream_cut_anywhere_across_2_to_the_32_is_the_one_call_result(L):
    c = lowpass_like_taps(L, 3 * L)
    iq = np.random.default_rng(L).integers(0, 256, 2 * CUT_N, dtype=np.uint8)
    whole, parts = fsea.Fir(c), fsea.Fir(c)
    d_in, d_out = fsea.DeviceBuffer(2 * CUT_N).upload(iq), Guarded(8 * CUT_N)
    for cps, ph in ((CPS, PHASE0), (1048575.999, -12345.678)):
        whole.reset()
        want = whole.run_u8_shifted(iq, cps, ph, CUT_START, flip=True)
        check(want, shift_ref.shifted_fir_reference(iq, 1, cps, ph, c, offset=CUT_START)[0], (L, cps))
        parts.reset()
        got, pos = [], 0
        for k in seeded_cuts(CUT_N, L, L):
            got.append(parts.run_u8_shifted(iq[2 * pos:2 * (pos + k)], cps, ph, CUT_START + pos, flip=True))
            pos += k
        assert np.array_equal(bits(np.concatenate(got)), bits(want)), (L, cps, "host pieces")
        # the device form: pieces at 16-byte boundaries of the input, each written at its own place
        parts.reset()
        d_out.upload(np.full(8 * CUT_N, FILL, np.uint8))
        pos = 0
        for k in seeded_cuts(CUT_N, L, L + 1, multiple=8):
            parts.run_shifted_device(d_in.ptr.value + 2 * pos, k, d_out.addr + 8 * pos, cps, ph, CUT_START + pos, flip=True)
            pos += k
        d_out.check((L, cps))
        assert np.array_equal(bits(d_out.payload(np.complex64, CUT_N)), bits(want)), (L, cps, "device pieces")
    d_in.free(), d_out.free(), whole.close(), parts.close()


# ---- the zoom -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,L,flip", [(3, 21, 0), (3, 512, 1), (16, 21, 1), (16, 512, 0)])
def test_zoom_pairs_and_rows_against_the_exact_reference_and_the_filter(D, L, flip):
    """fft_size 128, hop 64: 261 pairs, three rows.  Pairs against the exact reference; pairs == outputs 0, D, 2 D, ... of
    the shifted filter; rows == the rows of such a plan on the pairs (the row check of tests/test_gpu_zoom.py); device
    form == host form, into guarded payloads."""
    N, hop = 128, 64
    n = D * (2 * ZT + 5) + 1
    n_out, n_rows = n // D, (n // D - N) // hop + 1
    c = lowpass_like_taps(L, 100 * D + L)
    zoom, fir, plan = fsea.Zoom(c, D, N, hop), fsea.Fir(c), fsea.Plan(N, hop, fsea.MODE_MAG_F32)
    assert zoom.out_pairs(n) == n_out == 261 and zoom.out_rows(n) == n_rows == 3
    iq = np.random.default_rng(1000 * D + L).integers(0, 256, 2 * n, dtype=np.uint8)
    d_in = fsea.DeviceBuffer(2 * n).upload(iq)
    out = Outputs(rows=n_rows * zoom.row_bytes, pairs=8 * n_out)
    for offset, cps, ph in combos(n, residues=True):
        what = (D, L, flip, offset, cps, ph)
        zoom.reset()
        rows, pairs = zoom.run(iq, cps, ph, offset, flip=bool(flip), pairs=True)
        check(pairs, shift_ref.zoom_reference(iq, flip, cps, ph, c, D, offset=offset)[0], what)
        fir.reset()
        full = fir.run_u8_shifted(iq, cps, ph, offset, flip=bool(flip))
        assert np.array_equal(bits(pairs), bits(full[::D][:n_out])), what
        want_rows = plan.exec_host_f64(pairs.view(np.float32).astype(np.float64), n_rows)
        assert np.array_equal(rows.view(np.uint8), want_rows.view(np.uint8)), what
        zoom.reset()
        for g in out.g.values():
            g.upload(np.full(g.nbytes, FILL, np.uint8))
        zoom.run_device(d_in.ptr.value, n, out.addr("rows"), cps, ph, offset, flip=bool(flip), d_pairs_ptr=out.addr("pairs"))
        assert np.array_equal(bits(out.take("pairs", np.complex64, n_out, what)), bits(pairs)), what
        assert np.array_equal(bits(out.take("rows", np.float32, (n_rows, N), what)), bits(rows)), what
    d_in.free(), out.free(), zoom.close(), fir.close(), plan.close()


@pytest.mark.parametrize("D,L", [(3, 512), (16, 21)])
def test_zoom_stream_cut_at_multiples_of_d_across_2_to_the_32_is_the_one_call_result(D, L):
    c = lowpass_like_taps(L, 7 * D + L)
    iq = np.random.default_rng(D * L).integers(0, 256, 2 * CUT_N, dtype=np.uint8)
    zoom = fsea.Zoom(c, D, 128, 64)
    _, want = zoom.run(iq, CPS, PHASE0, CUT_START, flip=True, pairs=True)
    check(want, shift_ref.zoom_reference(iq, 1, CPS, PHASE0, c, D, offset=CUT_START)[0], (D, L))
    zoom.reset()
    got, pos = [], 0
    for k in seeded_cuts(CUT_N, L, D, multiple=D):
        got.append(zoom.run(iq[2 * pos:2 * (pos + k)], CPS, PHASE0, CUT_START + pos, flip=True, pairs=True)[1])
        pos += k
    assert np.array_equal(bits(np.concatenate(got)), bits(want))
    zoom.close()


# ---- the chain ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,flip,n_zero", [(21, 1, 0), (512, 0, 7)])
def test_chain_host_form_against_the_exact_reference(L, flip, n_zero):
    n = GRID_N
    c = lowpass_like_taps(L, 5 * L)
    chain = fsea.Chain(c)
    iq = np.random.default_rng(L + n_zero).integers(0, 256, 2 * n, dtype=np.uint8)
    for offset, cps, ph in combos(n):
        what = (L, flip, n_zero, offset, cps, ph)
        st = fsea.Chain.stage(flip=flip, cycles_per_sample=cps, phase0_cycles=ph, sample_offset=offset, n_zero=n_zero)
        chain.reset()
        got = chain.run(iq, st, pairs=True)["pairs"]
        assert chain.n_pairs == n + n_zero
        check(got, shift_ref.shifted_fir_reference(iq, flip, cps, ph, c, offset=offset, n_zero=n_zero)[0], what)
    chain.close()


@pytest.mark.parametrize("L,flip,n_zero", [(21, 0, 0), (512, 1, 10), (21, 1, 10)])
def test_chain_device_form_of_three_frames_against_the_exact_reference(L, flip, n_zero):
    """n a multiple of 8 and n_zero even, as the API asks; three frames span three tiles without zeros and end in a partial
    tile each with them.  The last position: sample_offset + 3 n == 2^52, the zeros not counted.  Frame by frame the
    bytes of three host runs of a second chain."""
    n, frames = 2056, 3
    per = n + n_zero
    c = lowpass_like_taps(L, 9 * L)
    device, host = fsea.Chain(c), fsea.Chain(c)
    iq = np.random.default_rng(L + n_zero + flip).integers(0, 256, 2 * n * frames, dtype=np.uint8)
    d_in = fsea.DeviceBuffer(iq.nbytes).upload(iq)
    out = Guarded(8 * per * frames)
    for offset, cps, ph in combos(n * frames):
        what = (L, flip, n_zero, offset, cps, ph)
        want, _ = shift_ref.chain_frames_reference(iq, n, frames, flip, cps, ph, c, offset, n_zero)
        device.reset()
        out.upload(np.full(out.nbytes, FILL, np.uint8))
        st = fsea.Chain.stage(flip=flip, cycles_per_sample=cps, phase0_cycles=ph, sample_offset=offset, n_zero=n_zero)
        device.run_device(d_in.ptr.value, n, frames, st, d_pairs=out.addr)
        out.check(what)
        got = out.payload(np.complex64, (frames, per))
        assert device.n_pairs == per
        host.reset()
        for f in range(frames):
            check(got[f], want[f], what + (f,))
            st = fsea.Chain.stage(flip=flip, cycles_per_sample=cps, phase0_cycles=ph, sample_offset=offset + f * n, n_zero=n_zero)
            single = host.run(iq[2 * n * f:2 * n * (f + 1)], st, pairs=True)["pairs"]
            assert np.array_equal(bits(got[f]), bits(single)), what + (f,)
    d_in.free(), out.free(), device.close(), host.close()


@pytest.mark.parametrize("n_zero", [0, 10])
def test_chain_frames_across_2_to_the_32_are_single_runs_with_the_offset_carried(n_zero):
    """Four frames of 2048 from 2^32 - 4100: 2^32 lies inside frame 2.  Without zeros the frames are one call of the
    filter over the stream; with them, four host runs of a second chain."""
    n, frames, L = CUT_N // 4, 4, 97
    per = n + n_zero
    c = lowpass_like_taps(L, 11)
    iq = np.random.default_rng(n_zero).integers(0, 256, 2 * CUT_N, dtype=np.uint8)
    chain, single, fir = fsea.Chain(c), fsea.Chain(c), fsea.Fir(c)
    d_in, out = fsea.DeviceBuffer(iq.nbytes).upload(iq), Guarded(8 * per * frames)
    st = fsea.Chain.stage(flip=True, cycles_per_sample=CPS, phase0_cycles=PHASE0, sample_offset=CUT_START, n_zero=n_zero)
    chain.run_device(d_in.ptr.value, n, frames, st, d_pairs=out.addr)
    out.check(n_zero)
    got = out.payload(np.complex64, (frames, per))
    want, _ = shift_ref.chain_frames_reference(iq, n, frames, 1, CPS, PHASE0, c, CUT_START, n_zero)
    for f in range(frames):
        check(got[f], want[f], (n_zero, f))
        st = fsea.Chain.stage(flip=True, cycles_per_sample=CPS, phase0_cycles=PHASE0, sample_offset=CUT_START + f * n, n_zero=n_zero)
        assert np.array_equal(bits(got[f]), bits(single.run(iq[2 * n * f:2 * n * (f + 1)], st, pairs=True)["pairs"])), (n_zero, f)
    if not n_zero:
        assert np.array_equal(bits(got.ravel()), bits(fir.run_u8_shifted(iq, CPS, PHASE0, CUT_START, flip=True)))
    d_in.free(), out.free(), chain.close(), single.close(), fir.close()


# ---- inputs between two fills, above 2^32 ---------------------------------------------------------------------------

def test_inputs_above_2_to_the_32_are_read_inside_their_bounds():
    """As tests/test_gpu_bounds.py, at sample_offset 2^40 + 3: each device form once with its input between bands of
    0x00 and once of 0xFF, in a fresh state; both equal the host form of another object bit for bit."""
    offset, L, D = ABOVE + 3, 51, 3
    c = lowpass_like_taps(L, L)
    rng = np.random.default_rng(40)
    n_fir, n_chain, frames, n_zero, n_zoom = GRID_N, 2056, 3, 10, D * (2 * ZT + 5) + 1
    iq_fir = rng.integers(0, 256, 2 * n_fir, dtype=np.uint8)
    iq_chain = rng.integers(0, 256, 2 * n_chain * frames, dtype=np.uint8)
    iq_zoom = rng.integers(0, 256, 2 * n_zoom, dtype=np.uint8)
    fir, chain, zoom = fsea.Fir(c), fsea.Chain(c), fsea.Zoom(c, D, 128, 64)
    want_fir = fir.run_u8_shifted(iq_fir, CPS, PHASE0, offset, flip=True)
    want_chain = [chain.run(iq_chain[2 * n_chain * f:2 * n_chain * (f + 1)],
                            fsea.Chain.stage(True, CPS, PHASE0, offset + f * n_chain, n_zero), pairs=True)["pairs"] for f in range(frames)]
    want_rows, want_pairs = zoom.run(iq_zoom, CPS, PHASE0, offset, flip=True, pairs=True)
    for fill in INPUT_FILLS:
        fir.reset(), chain.reset(), zoom.reset()
        (g_f, d_f), (g_c, d_c), (g_z, d_z) = fenced(iq_fir, fill), fenced(iq_chain, fill), fenced(iq_zoom, fill)
        out = Outputs(fir=8 * n_fir, chain=8 * (n_chain + n_zero) * frames, rows=want_rows.nbytes, pairs=want_pairs.nbytes)
        fir.run_shifted_device(d_f, n_fir, out.addr("fir"), CPS, PHASE0, offset, flip=True)
        chain.run_device(d_c, n_chain, frames, fsea.Chain.stage(True, CPS, PHASE0, offset, n_zero), d_pairs=out.addr("chain"))
        zoom.run_device(d_z, n_zoom, out.addr("rows"), CPS, PHASE0, offset, flip=True, d_pairs_ptr=out.addr("pairs"))
        same(out.take("fir", np.complex64, n_fir, fill), want_fir, (fill, "fir"))
        same(out.take("chain", np.complex64, (frames, n_chain + n_zero), fill), np.stack(want_chain), (fill, "chain"))
        same(out.take("pairs", np.complex64, want_pairs.shape, fill), want_pairs, (fill, "zoom pairs"))
        same(out.take("rows", want_rows.dtype, want_rows.shape, fill), want_rows, (fill, "zoom rows"))
        for g in (g_f, g_c, g_z):
            g.check((fill, "input"))
            g.free()
        out.free()
    fir.close(), chain.close(), zoom.close()


# ---- refusals and the fields a shift == 0 ignores -------------------------------------------------------------------

REFUSED = [(8, 1, dict(n_zero=0, **bad)) for _, bad in BAD_SHIFTS]
REFUSED += [(8, 3, dict(n_zero=2, offset=LIMIT - 16)),         # frames 0 and 1 end at or below 2^52, frame 2 does not
            (8, 3, dict(n_zero=2, cps=np.nan))]


@pytest.mark.parametrize("n,n_frames,bad", REFUSED)
def test_a_refused_chain_call_writes_nothing_and_the_stream_goes_on(n, n_frames, bad):
    """A good call, the refused call in both forms, then: n_pairs, the resident pairs and its image as before, the outputs
    of the refused calls untouched, and the next good call the bytes of a second chain that never saw the refused one."""
    L_ = fsea.hip_lib()
    c = lowpass_like_taps(51, 51)
    rng = np.random.default_rng(n_frames)
    first, more = rng.integers(0, 256, 2 * 1000, dtype=np.uint8), rng.integers(0, 256, 2 * 300, dtype=np.uint8)
    junk = rng.integers(0, 256, 2 * n * n_frames, dtype=np.uint8)
    seen, unseen = fsea.Chain(c), fsea.Chain(c)
    good = fsea.Chain.stage(flip=True, cycles_per_sample=CPS, phase0_cycles=PHASE0, sample_offset=ABOVE + 3, n_zero=4)
    before = seen.run(first, good, points=True, pairs=True)
    unseen.run(first, good)
    assert seen.n_pairs == 1004
    st = fsea.ChainStage(1, 1, bad.get("cps", CPS), bad.get("phase0", 0.0), bad.get("offset", 0), bad["n_zero"])
    per = n + bad["n_zero"]
    if n_frames == 1:
        host_out = {k: np.full(size, FILL, np.uint8) for k, size in (("points", 65536), ("lines", 65536), ("pairs", 8 * per))}
        o = fsea.ChainOutputs(host_out["points"].ctypes.data, host_out["lines"].ctypes.data, 1, per, host_out["pairs"].ctypes.data)
        assert L_.fsea_chain_run_host(seen._p, junk.ctypes.data, n, ctypes.byref(st), ctypes.byref(o)) == FSEA_EINVAL
        assert all(np.all(a == FILL) for a in host_out.values())
        assert seen.n_pairs == 1004
    d_in = fsea.DeviceBuffer(max(junk.nbytes, 16)).upload(junk)
    out = Outputs(points=65536 * n_frames, lines=65536 * n_frames, pairs=8 * per * n_frames)
    with pytest.raises(fsea.FseaError):
        seen.run_device(d_in.ptr.value, n, n_frames, st, d_points=out.addr("points"), d_lines=out.addr("lines"), lines_m=1,
                        d_pairs=out.addr("pairs"))
    for name, g in out.g.items():
        g.check((bad, name))
        assert np.all(g.payload(np.uint8, g.nbytes) == FILL), (bad, name)
    assert seen.n_pairs == 1004
    after = seen.fetch(points=True, pairs=True)
    assert np.array_equal(bits(after["pairs"]), bits(before["pairs"])) and np.array_equal(after["points"], before["points"])
    nxt = fsea.Chain.stage(flip=True, cycles_per_sample=CPS, phase0_cycles=PHASE0, sample_offset=ABOVE + 1003, n_zero=0)
    got, want = seen.run(more, nxt, points=True, pairs=True), unseen.run(more, nxt, points=True, pairs=True)
    assert np.array_equal(bits(got["pairs"]), bits(want["pairs"])) and np.array_equal(got["points"], want["points"])
    d_in.free(), out.free(), seen.close(), unseen.close()


def test_the_last_admissible_chain_calls_are_not_refused():
    """sample_offset + n_frames n_samples == 2^52 with zero samples behind every frame: they do not count (include/fsea.h)."""
    n, frames, n_zero = 2056, 3, 10
    c = lowpass_like_taps(21, 1)
    iq = np.random.default_rng(52).integers(0, 256, 2 * n * frames, dtype=np.uint8)
    chain = fsea.Chain(c)
    got = chain.run(iq[:2 * n], fsea.Chain.stage(False, CPS, PHASE0, LIMIT - n, n_zero), pairs=True)["pairs"]
    check(got, shift_ref.shifted_fir_reference(iq[:2 * n], 0, CPS, PHASE0, c, offset=LIMIT - n, n_zero=n_zero)[0], "host")
    with pytest.raises(fsea.FseaError, match="sample_offset"):
        chain.run(iq[:2 * n], fsea.Chain.stage(False, CPS, PHASE0, LIMIT - n + 1, n_zero), pairs=True)
    chain.close()


@pytest.mark.parametrize("n_frames", [1, 3])
def test_without_a_shift_the_other_stage_fields_are_ignored(n_frames):
    """shift == 0 with NaN, infinities and positions beyond the limit in the other fields: the unshifted result, bit for
    bit, host and device form."""
    n = 2056
    c = lowpass_like_taps(51, 3)
    iq = np.random.default_rng(n_frames).integers(0, 256, 2 * n * n_frames, dtype=np.uint8)
    plain, chain = fsea.Chain(c), fsea.Chain(c)
    d_in, out = fsea.DeviceBuffer(iq.nbytes).upload(iq), Guarded(8 * n * n_frames)
    L_ = fsea.hip_lib()
    for _, bad in BAD_SHIFTS + [(b"", dict(cps=np.nan, phase0=-np.inf, offset=(1 << 64) - 1))]:
        st = fsea.ChainStage(1, 0, bad.get("cps", 0.01), bad.get("phase0", 0.0), bad.get("offset", 0), 0)
        plain.reset(), chain.reset()
        want = plain.run(iq, fsea.Chain.stage(flip=True), pairs=True)["pairs"]
        check(want, fir_reference(u8_to_complex(iq, 1), c)[0], bad)
        got = chain.run(iq, st, pairs=True)["pairs"]
        assert np.array_equal(bits(got), bits(want)), bad
        chain.reset()
        out.upload(np.full(out.nbytes, FILL, np.uint8))
        chain.run_device(d_in.ptr.value, n, n_frames, st, d_pairs=out.addr)
        out.check(bad)
        assert np.array_equal(bits(out.payload(np.complex64, n * n_frames)), bits(want)), bad
    assert L_.fsea_chain_n_pairs(chain._p) == n
    d_in.free(), out.free(), plain.close(), chain.close()


# ---- the host blocks at a consumed of 2^44 --------------------------------------------------------------------------

CONSUMED, BLOCK_PAIRS = 1 << 44, 4096


def _iq_chain_block(L, data, kind):
    """One block through a fresh nrf_iq_chain (5 MHz, 60 kHz, 97 taps, shifter at -600 kHz: -0.12 cycles per sample) whose
    shifter has consumed 2^44 samples; the 2 * 4096 pairs of its result."""
    chain = L.nrf_iq_chain_new(5000000, 60000, 97)
    L.nrf_iq_chain_set_shifter(chain, -600000)
    view = ctypes.cast(chain, ctypes.POINTER(nrf.NrfIqChain)).contents
    assert (view.sample_rate, view.length, view.shifting, view.freq_offset, view.consumed) == (5000000, 97, 1, -600000, 0)
    view.consumed = CONSUMED
    if kind == "u8":
        buf = L.nut_buffer_new_u8(BLOCK_PAIRS, 2, data.ctypes.data)
    else:
        f64 = data / 256.0
        buf = L.nut_buffer_new_f64(BLOCK_PAIRS, 2, f64.ctypes.data)
    L.nrf_iq_chain_process(chain, buf)
    assert view.consumed == CONSUMED + BLOCK_PAIRS
    out = L.nrf_iq_chain_get_buffer(chain)
    assert out.contents.length == 2 * BLOCK_PAIRS
    v = nrf.buffer_to_numpy(L, out)
    y = v[0::2] + 1j * v[1::2]
    L.nut_buffer_free(out), L.nut_buffer_free(buf), L.nrf_iq_chain_free(chain)
    return y


@pytest.fixture(scope="module")
def block_at_2_44():
    data = np.random.default_rng(44).integers(0, 256, 2 * BLOCK_PAIRS, dtype=np.uint8)
    assert -600000 / 5000000 == CPS
    c = fsea.lowpass_taps(5e6, 60e3, 97)
    want, _ = shift_ref.shifted_fir_reference(data, 0, CPS, 0.0, c, offset=CONSUMED, n_zero=BLOCK_PAIRS)
    return data, want


def test_nrf_iq_chain_u8_block_at_2_to_the_44_against_the_exact_reference(block_at_2_44):
    data, want = block_at_2_44
    y = _iq_chain_block(nrf.nrf_lib(), data, "u8")
    err = float(np.max(np.abs(y - want)))
    print("nrf_iq_chain U8 at consumed 2^44: max |delta| %.3e" % err)
    assert err <= MAX_ABS, err


def test_nrf_iq_chain_f64_block_at_2_to_the_44_against_the_exact_reference_and_the_u8_block(block_at_2_44):
    """The F64 path rotates on the host.  With one rounded product for the phase it stood 1e-4 cycles off here (measured
    before the fixes: max |delta| 9.8e-5 against the exact reference behind the 60 kHz low-pass, 1.3e-4 against the U8
    pass, whose kernel was off the other way); with the two-term reduction both inputs of the block see the same phase.
    After: 3.6e-7 against the exact reference."""
    data, want = block_at_2_44
    L = nrf.nrf_lib()
    y = _iq_chain_block(L, data, "f64")
    err = float(np.max(np.abs(y - want)))
    both = float(np.max(np.abs(y - _iq_chain_block(L, data, "u8"))))
    print("nrf_iq_chain F64 at consumed 2^44: max |delta| %.3e; against the U8 pass %.3e" % (err, both))
    assert err <= MAX_ABS, err
    assert both <= 2 * MAX_ABS, both


def test_nrf_zoom_fft_block_at_2_to_the_44_against_the_exact_reference():
    """The block's rows are fsea_zoom's at sample_offset = consumed, bit for bit (as tests/test_gpu_zoom.py at small
    positions), those are the plan's rows on the pairs, and the pairs are held to the exact reference."""
    L = nrf.nrf_lib()
    rate, offset_hz, D, N, H = 10000000, -1200000, 16, 128, 4
    data = np.random.default_rng(45).integers(0, 256, 2 * BLOCK_PAIRS, dtype=np.uint8)
    z = L.nrf_zoom_fft_new(rate, offset_hz, D, 200000, 97, N, H)
    view = ctypes.cast(z, ctypes.POINTER(nrf.NrfZoomFft)).contents
    assert (view.sample_rate, view.freq_offset, view.decimation, view.fft_size, view.fft_history_size, view.consumed) == \
        (rate, offset_hz, D, N, H, 0)
    view.consumed = CONSUMED
    buf = L.nut_buffer_new_u8(BLOCK_PAIRS, 2, data.ctypes.data)
    L.nrf_zoom_fft_process(z, buf)
    assert view.consumed == CONSUMED + BLOCK_PAIRS
    hist = L.nrf_zoom_fft_get_buffer(z)
    got = nrf.buffer_to_numpy(L, hist).reshape(H, N)
    c = fsea.lowpass_taps(rate, 200000, 97)
    zoom = fsea.Zoom(c, D, N)
    rows, pairs = zoom.run(data, offset_hz / rate, 0.0, CONSUMED, pairs=True)
    assert rows.shape == (2, N) and np.array_equal(got[:2], rows[::-1].astype(np.float64)) and not got[2:].any()
    check(pairs, shift_ref.zoom_reference(data, 0, offset_hz / rate, 0.0, c, D, offset=CONSUMED)[0], "zoom block")
    zoom.reset()
    assert not np.array_equal(zoom.run(data, offset_hz / rate, 0.0, 0)[0], rows)          # the position matters
    L.nut_buffer_free(hist), L.nut_buffer_free(buf), L.nrf_zoom_fft_free(z), zoom.close()
