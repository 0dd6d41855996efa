"""GPU tier: the polyphase filter bank (fsea_pfb_*, kernels fsea_pfb_frames_u8 and fsea_pfb_transpose), the nrf_pfb_fft
block and fsea-pfb-fft.

Bit identity, no tolerance: the rows of every mode are fsea_exec_f64_host of an identically configured plan on the frames
widened to double; the series is the rows transposed; a frame entry is the output of the full-rate filter (fsea.Fir) with
the branch's taps at their places and zeros elsewhere (a zero tap leaves an FMA chain's bits alone); a stream cut at
multiples of D is the one-call result.
Against double: the frames against tests/pfb_ref.py's pfb_frames_reference within tests/test_gpu_fir.py's MAX_ABS = 1e-5 and
MAX_REL = 1e-6 -- every entry is one FMA chain of at most 16 taps with sum |c| < 2 over a branch (tests/test_pfb_host.py),
an f32 emulation with two roundings per tap stays below 1e-7 relative.  COMPLEX rows against pfb_direct at relative L2 <=
2e-6, the zoom's budget: the input's 1e-6 plus the transform's 1e-6.  pfb_direct costs F L operations per channel: up to
128 channels all of them are compared, above that 32 of them (the centre, the edges and 26 drawn at random) -- every
column of those sizes is still held by the two bit identities and the frames' bound.
One reference per (case, taps, flip) over the longest call serves every shorter one: frame t of a call from reset reads
the call's first t D + 1 samples only."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import parity, pfb_ref
from tests.conftest import ROOT
from tests.test_gpu_fir import check

pytestmark = pytest.mark.gpu

POW2 = [(32, 4, 1), (32, 16, 4), (64, 8, 2), (128, 8, 1), (1024, 8, 1), (1024, 16, 4), (16384, 4, 2)]
BLUESTEIN = [(6, 3, 1), (12, 4, 4), (50, 4, 2)]
CASES = POW2 + BLUESTEIN
BIN = os.path.join(ROOT, "frequensea_amd", "bin")
FSEA_EINVAL = -1
ALL_MODES = [fsea.MODE_MAG_F32, fsea.MODE_DB10_U8, fsea.MODE_DB5_U8_DCFIX, fsea.MODE_COMPLEX_F32, fsea.MODE_MAG_NODC_F32,
             fsea.MODE_DB_F32]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32 if a.dtype == np.float32 else np.uint8)


def frame_counts(M, P, q):
    """F: 0, 1, 2, P, 63, 64, 65, 129 and one below, at and one above one and two tiles; at M = 16384 only F <= 5."""
    _, T = pfb_ref.tile_shape(M, P, q)
    fs = sorted({0, 1, 2, P, 63, 64, 65, 129, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1})
    return [f for f in fs if f <= 5] if M == 16384 else fs


def make_taps(kind, M, P):
    return fsea.pfb_prototype(M, P) if kind == "prototype" else pfb_ref.branch_normalised_taps(M, P, 10 * M + P)


def direct_columns(M):
    if M <= 128:
        return np.arange(M)
    rng = np.random.default_rng(M)
    return np.unique(np.concatenate([[0, 1, M // 2 - 1, M // 2, M // 2 + 1, M - 1], rng.integers(0, M, 26)]))


@functools.lru_cache(maxsize=None)
def reference(M, P, q, kind, flip):
    """The longest call of a case: its bytes, the frames in double and the direct rows (of direct_columns)."""
    D = M // q
    n = max(frame_counts(M, P, q)) * D + D - 1
    iq = np.random.default_rng(1000 * M + 10 * P + q + flip).integers(0, 256, 2 * n, dtype=np.uint8)
    c = make_taps(kind, M, P)
    frames, _ = pfb_ref.pfb_frames_reference(iq, flip, c, M, D)
    rows, _ = pfb_ref.pfb_direct(iq, flip, c, M, D, columns=direct_columns(M))
    return iq, frames, rows


@pytest.mark.parametrize("kind,flip", [("random", 0), ("prototype", 1)])
@pytest.mark.parametrize("M,P,q", CASES)
def test_frames_and_complex_rows_against_the_restatement(M, P, q, kind, flip):
    """From reset, one call per frame count; the left-over is 0, D - 1 or D / 2 samples in turn (n no multiple of D), and
    F = 0 with n = D - 1 is the call below D."""
    D = M // q
    iq, want_frames, want_rows = reference(M, P, q, kind, flip)
    cols = direct_columns(M)
    pfb = fsea.Pfb(make_taps(kind, M, P), M, q, fsea.MODE_COMPLEX_F32)
    worst = 0.0
    for i, F in enumerate(frame_counts(M, P, q)):
        n = F * D + (0, D - 1, D // 2)[i % 3] if F else D - 1
        pfb.reset()
        assert pfb.out_frames(n) == F
        rows, frames, _ = pfb.run(iq[:2 * n], flip=bool(flip), frames=True)
        assert rows.shape == frames.shape == (F, M)
        check(frames, want_frames[:F], (M, P, q, kind, flip, F))
        if F:
            rel = float(np.linalg.norm(rows[:, cols] - want_rows[:F]) / np.linalg.norm(want_rows[:F]))
            worst = max(worst, rel)
            assert rel <= 2e-6, (M, P, q, kind, flip, F, rel)
    print("M %d P %d q %d %s flip %d: COMPLEX rows relative L2 at most %.3e" % (M, P, q, kind, flip, worst))
    pfb.close()


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("M,P,q", [(64, 8, 2), (1024, 8, 1), (50, 4, 2)])
def test_rows_are_the_plans_rows_on_the_frames(M, P, q, mode):
    D = M // q
    n = 37 * D + 3
    iq = np.random.default_rng(M + mode).integers(0, 256, 2 * n, dtype=np.uint8)
    pfb, plan = fsea.Pfb(fsea.pfb_prototype(M, P), M, q, mode), fsea.Plan(M, M, mode)
    rows, frames, _ = pfb.run(iq, flip=True, frames=True)
    assert rows.shape == (37, M) and pfb.row_bytes == plan.row_bytes
    want = plan.exec_host_f64(frames.view(np.float32).astype(np.float64), 37)
    assert np.array_equal(rows.view(np.uint8), want.view(np.uint8)), (M, P, q, mode)
    pfb.close()
    plan.close()


@pytest.mark.parametrize("flip", [0, 1])
def test_a_frame_entry_is_the_full_rate_filters_output_with_the_branchs_taps(flip):
    """(M, P, q) = (8, 4, 2) from reset: frames[t][(r + t D) % M] = Fir(c_r).run_u8(iq)[t D], c_r[k] = c[k] where k = r mod M."""
    M, P, q, D = 8, 4, 2, 4
    c = pfb_ref.branch_normalised_taps(M, P, 3)
    n = 41 * D + 1
    iq = np.random.default_rng(8 + flip).integers(0, 256, 2 * n, dtype=np.uint8)
    pfb = fsea.Pfb(c, M, q, fsea.MODE_COMPLEX_F32)
    _, frames, _ = pfb.run(iq, flip=bool(flip), frames=True)
    pfb.close()
    for r in range(M):
        c_r = np.where(np.arange(M * P) % M == r, c, 0.0)
        fir = fsea.Fir(c_r)
        full = fir.run_u8(iq, flip=bool(flip))
        fir.close()
        for t in range(41):
            assert frames[t][(r + t * D) % M] == full[t * D], (r, t)


@pytest.mark.parametrize("M,P,q", [(32, 4, 1), (128, 8, 1), (1024, 16, 4), (50, 4, 2)])
def test_series_is_the_rows_transposed(M, P, q):
    D = M // q
    for F in (1, 31, 32, 33, 70):
        iq = np.random.default_rng(M + F).integers(0, 256, 2 * (F * D + 1), dtype=np.uint8)
        pfb = fsea.Pfb(fsea.pfb_prototype(M, P), M, q, fsea.MODE_COMPLEX_F32)
        rows, _, series = pfb.run(iq, series=True)
        assert series.shape == (M, F) and np.array_equal(bits(series), bits(rows.T)), (M, P, q, F)
        pfb.close()


@pytest.mark.parametrize("M,P,q", [(64, 8, 2), (32, 16, 4), (1024, 8, 1), (12, 4, 4)])
def test_a_stream_cut_at_multiples_of_d_is_the_one_call_result(M, P, q):
    """Cuts at multiples of D: one no multiple of M where q > 1, one shorter than L - 1; then repeat, reset, and a second
    call after a length that is no multiple of D against the restatement with the carried tail and s0."""
    D, L = M // q, M * P
    _, T = pfb_ref.tile_shape(M, P, q)
    cuts = [D * (2 * T + 5), D * (q + 1), D * 37, D * max((L - 1) // D - 1, 1)]
    assert q == 1 or (cuts[1] % M and cuts[3] < L - 1)
    n = sum(cuts)
    c = pfb_ref.branch_normalised_taps(M, P, M + q)
    iq = np.random.default_rng(M * P).integers(0, 256, 2 * n, dtype=np.uint8)
    pfb = fsea.Pfb(c, M, q, fsea.MODE_COMPLEX_F32)
    rows, want, _ = pfb.run(iq, flip=True, frames=True)
    check(want, pfb_ref.pfb_frames_reference(iq, 1, c, M, D)[0], (M, P, q))
    pfb.reset()
    got, got_rows, pos = [], [], 0
    for k in cuts:
        r, f, _ = pfb.run(iq[2 * pos:2 * (pos + k)], flip=True, frames=True)
        got.append(f)
        got_rows.append(r)
        pos += k
    assert np.array_equal(bits(np.concatenate(got)), bits(want)) and np.array_equal(bits(np.concatenate(got_rows)), bits(rows))
    again = pfb.run(iq, flip=True, frames=True)               # not reset: the tail and the position of the stream's end
    assert not np.array_equal(again[1][:2], want[:2])
    pfb.reset()
    again = pfb.run(iq, flip=True, frames=True)               # reset: the first result
    assert np.array_equal(bits(again[1]), bits(want)) and np.array_equal(bits(again[0]), bits(rows))
    # a length that is no multiple of D, then a second call: its frames start at its own sample 0
    pfb.reset()
    n1 = 9 * D + D // 2 + 1
    pfb.run(iq[:2 * n1], flip=True)
    _, got2, _ = pfb.run(iq[2 * n1:2 * (n1 + 11 * D)], flip=True, frames=True)
    _, tail = pfb_ref.pfb_frames_reference(iq[:2 * n1], 1, c, M, D)
    check(got2, pfb_ref.pfb_frames_reference(iq[2 * n1:2 * (n1 + 11 * D)], 1, c, M, D, tail, n1)[0], (M, P, q, "second call"))
    pfb.close()


def test_device_form_on_a_callers_stream_equals_the_host_form():
    M, P, q = 128, 8, 2
    D = M // q
    c = fsea.pfb_prototype(M, P)
    n = 75 * D + 5
    iq = np.random.default_rng(3).integers(0, 256, 2 * n, dtype=np.uint8)
    pfb = fsea.Pfb(c, M, q, fsea.MODE_COMPLEX_F32)
    rows, frames, series = pfb.run(iq, flip=True, frames=True, series=True)
    sync = fsea.Plan(M)                          # fsea_stream_synchronize wants a plan for its device
    st = fsea.Stream()
    d_in = fsea.DeviceBuffer(iq.nbytes).upload(iq)
    d_rows, d_frames, d_series = (fsea.DeviceBuffer(rows.nbytes) for _ in range(3))
    for want_frames, want_series in ((True, True), (False, True), (True, False), (False, False)):
        pfb.reset()
        pfb.run_device(d_in.ptr.value, n, d_rows.ptr.value, flip=True, d_frames_ptr=d_frames.ptr.value if want_frames else None,
                       d_series_ptr=d_series.ptr.value if want_series else None, stream=st)
        sync.synchronize(st)
        assert np.array_equal(bits(d_rows.download(np.complex64, rows.shape)), bits(rows))
        if want_frames:
            assert np.array_equal(bits(d_frames.download(np.complex64, frames.shape)), bits(frames))
        if want_series:
            assert np.array_equal(bits(d_series.download(np.complex64, series.shape)), bits(series))
        for b in (d_rows, d_frames, d_series):
            b.upload(np.zeros_like(rows))
    # what needs a real object to be refused: rows that have nowhere to go, a series outside COMPLEX mode
    L_ = fsea.hip_lib()
    assert L_.fsea_pfb_run_device(pfb._p, d_in.ptr, n, 1, None, None, None, None) == FSEA_EINVAL
    assert L_.fsea_pfb_run_host(pfb._p, iq.ctypes.data, n, 1, None, None, None) == FSEA_EINVAL
    assert L_.fsea_pfb_run_host(pfb._p, iq.ctypes.data, D - 1, 1, None, None, None) == 0   # no frame
    mag = fsea.Pfb(c, M, q, fsea.MODE_MAG_F32)
    assert L_.fsea_pfb_run_device(mag._p, d_in.ptr, n, 1, d_rows.ptr, None, d_series.ptr, None) == FSEA_EINVAL
    assert L_.fsea_pfb_run_host(mag._p, iq.ctypes.data, n, 1, rows.ctypes.data, None, rows.ctypes.data) == FSEA_EINVAL
    mag.close()
    for b in (d_in, d_rows, d_frames, d_series):
        b.free()
    st.close()
    sync.close()
    pfb.close()


def test_a_failed_create_leaves_nothing_and_the_plans_status_is_the_banks():
    L_ = fsea.hip_lib()
    c = fsea.pfb_prototype(64, 4)
    h = ctypes.c_void_p()
    plan_rc = L_.fsea_plan_create(ctypes.byref(h), 64, 64, 9, 0)                      # a mode no plan has
    plan_text = L_.fsea_last_error_string()
    assert plan_rc != 0 and not h.value
    rc = L_.fsea_pfb_create(ctypes.byref(h), c.ctypes.data, 64, 4, 1, 9, 0)
    assert rc == plan_rc and not h.value and L_.fsea_last_error_string() == plan_text
    assert L_.fsea_pfb_create(ctypes.byref(h), c.ctypes.data, 64, 4, 1, 0, 4096) != 0 and not h.value   # no such device
    pfb = fsea.Pfb(c, 64, 1, fsea.MODE_COMPLEX_F32)                                     # and a valid one works after them
    iq = np.random.default_rng(0).integers(0, 256, 2 * 64 * 9, dtype=np.uint8)
    _, frames, _ = pfb.run(iq, frames=True)
    check(frames, pfb_ref.pfb_frames_reference(iq, 0, c, 64, 64)[0])
    pfb.close()


def test_the_bank_does_not_leak_where_a_rectangular_row_does():
    """tests/test_pfb_host.py's leakage statement through fsea.Pfb and fsea.Plan, the same thresholds."""
    M, P, frames = 128, 8, 72
    raw = pfb_ref.tone_bytes(M, frames)
    pfb = fsea.Pfb(fsea.pfb_prototype(M, P), M, 1, fsea.MODE_MAG_F32)
    rows, _, _ = pfb.run(raw, flip=True)
    pfb.close()
    top, ratio = pfb_ref.leakage(rows[8:].astype(np.float64).mean(axis=0))
    print("bank: largest columns %s, leakage %.3e" % (sorted(top), ratio))
    assert top == {74, 75} and ratio <= 1e-2
    plan = fsea.Plan(M, M, fsea.MODE_MAG_F32)
    rect = plan.exec_host(raw, flip=True)
    plan.close()
    top, ratio = pfb_ref.leakage(rect[8:].astype(np.float64).mean(axis=0))
    print("rectangular: largest columns %s, leakage %.3e" % (sorted(top), ratio))
    assert top == {74, 75} and ratio >= 0.1


def _history(L, p, n_fft, rows):
    buf = L.nrf_pfb_fft_get_buffer(p)
    assert buf.contents.length == n_fft * rows and buf.contents.channels == 1 and buf.contents.type == nrf.NUT_BUFFER_F64
    h = nrf.buffer_to_numpy(L, buf).reshape(rows, n_fft)
    L.nut_buffer_free(buf)
    return h


def test_host_block_scrolls_the_banks_rows_into_its_history(golden_all):
    L = nrf.nrf_lib()
    N, H, P = 128, 2048, 8
    block = np.ascontiguousarray(golden_all["block__raw"] ^ 0x80)
    n = block.size // 2
    p = L.nrf_pfb_fft_new(N, H, P)
    pfb = fsea.Pfb(fsea.pfb_prototype(N, P), N, 1, fsea.MODE_MAG_F32)
    assert not _history(L, p, N, H).any()
    want = np.zeros((H, N))
    for k in range(3):
        buf = L.nut_buffer_new_u8(n, 2, block.ctypes.data)
        L.nrf_pfb_fft_process(p, buf)
        L.nut_buffer_free(buf)
        rows, _, _ = pfb.run(block)
        assert rows.shape == (n // N, N)
        want = np.concatenate([rows[::-1].astype(np.float64), want])[:H]    # newest first
        assert np.array_equal(_history(L, p, N, H), want), k
    L.nrf_pfb_fft_free(p)
    pfb.close()
    # a history shorter than a block's rows keeps the newest
    pfb = fsea.Pfb(fsea.pfb_prototype(N, P), N, 1, fsea.MODE_MAG_F32)
    rows, _, _ = pfb.run(block)
    pfb.close()
    p = L.nrf_pfb_fft_new(N, 10, P)
    buf = L.nut_buffer_new_u8(n, 2, block.ctypes.data)
    L.nrf_pfb_fft_process(p, buf)
    L.nut_buffer_free(buf)
    assert np.array_equal(_history(L, p, N, 10), rows[::-1][:10].astype(np.float64))
    L.nrf_pfb_fft_free(p)


def test_host_block_refuses_an_f64_buffer():
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n"
            "p = L.nrf_pfb_fft_new(128, 8, 8)\n"
            "L.nrf_pfb_fft_process(p, L.nut_buffer_new_f64(4096, 2, None))\n"
            "print('returned')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PFB FFT fatal error" in r.stderr and "F64" in r.stderr


def test_tool_writes_the_banks_rows_a_series_and_prints_its_numbers(tmp_path):
    from PIL import Image
    M, P, q, K = 256, 8, 2, 150
    raw = pfb_ref.tone_bytes(M, 300, offset_channels=22.25, amp=60.0, sigma=10.0, seed=4)
    raw.tofile(tmp_path / "tone.raw")
    out, ser = tmp_path / "pfb.png", tmp_path / "ch.f32"
    r = subprocess.run([os.path.join(BIN, "fsea-pfb-fft"), str(tmp_path / "tone.raw"), "--rate", "8000000", "--channels",
                        str(M), "--oversampling", str(q), "--out", str(out), "--channel", str(K), "--series", str(ser)],
                       capture_output=True, text=True, check=True, timeout=300)
    c = fsea.pfb_prototype(M, P)                                                    # --taps 8 is the default
    pfb = fsea.Pfb(c, M, q, fsea.MODE_DB10_U8)
    rows, _, _ = pfb.run(raw, flip=True)
    pfb.close()
    with Image.open(out) as im:
        got = np.array(im)
    assert got.dtype == np.uint8 and np.array_equal(got, rows) and rows.shape == (600, M)
    assert "rows 600" in r.stdout and "channel width 31250.000000 Hz" in r.stdout and "row rate 62500.000000 Hz" in r.stdout
    pfb = fsea.Pfb(c, M, q, fsea.MODE_COMPLEX_F32)
    spectra, _, _ = pfb.run(raw, flip=True)
    pfb.close()
    assert np.array_equal(bits(np.fromfile(ser, dtype=np.complex64)), bits(spectra[:, K]))
