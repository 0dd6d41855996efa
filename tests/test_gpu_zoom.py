"""GPU tier: the zoom spectrum (fsea_zoom_*, kernel fsea_shift_decim_u8), the nrf_zoom_fft block and fsea-zoom-fft.

Bit identity, no tolerance: the decimated pairs are outputs 0, D, 2 D, ... of fsea_fir_u8_shifted_host with the same taps,
state and arguments (the same staging arithmetic, one FMA chain per output, taps ascending), and the rows are
fsea_exec_f64_host of an identically configured plan on those pairs widened to double (widening then narrowing is exact,
frames are independent of the launch's shape).
Against double: the pairs against tests/test_zoom_host.py's zoom_reference within tests/test_gpu_fir.py's MAX_ABS = 1e-5 and
MAX_REL = 1e-6 -- every output is one of the sums those bounds were derived for.  COMPLEX rows against numpy.fft of
zoom_reference with the (-1)^n centring at relative L2 <= 2e-6: the transform is an isometry up to sqrt(N), so the input's
1e-6 plus the FFT's own REL_L2_TOL = 1e-6 of tests/parity.py.  MAG and dB rows are not held to an end-to-end bound (the DC
fix removes most of a row's norm): their deviation is printed, bit identity to the existing path carries them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import parity
from tests.conftest import ROOT
from tests.test_gpu_fir import check, random_taps
from tests.test_zoom_host import zoom_reference

pytestmark = pytest.mark.gpu

T = fsea.ZOOM_TILE_OUTPUTS
CASES = [(1, 21), (2, 1), (2, 97), (3, 41), (5, 2), (8, 97), (16, 97), (16, 512), (25, 97), (64, 512)]
CPS, PHASE0, OFFSET = -1.2e6 / 10e6, 0.3, 1234563      # the offset is no multiple of 8
BIN = os.path.join(ROOT, "frequensea_amd", "bin")
FSEA_EINVAL = -1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lowpass_like_taps(L, seed):
    """Non-symmetric positive taps with sum c = sum |c| = 1: S = 1 and a DC gain of 1, so that rms(y) >= 0.5 on offset-binary
    input -- the premises (S < 2, rms(y) >= ~0.3) under which tests/test_gpu_fir.py derives MAX_ABS and MAX_REL.  Taps of
    random sign (random_taps) have a DC gain near 0 and rms(y) ~ 0.04 at L = 512: there the f32 rounding of a call of three
    outputs measured 1.006e-6 relative (4.5e-8 absolute) with pairs bit-identical to the full-rate filter's."""
    c = np.abs(np.random.default_rng(seed).standard_normal(L)) + 1e-3
    return c / c.sum()


def lengths(D, L):
    """n with n_out one below, at and one above one and two tiles; not a multiple of D; below D; below L - 1; zero."""
    ns = [m * D for m in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)]
    ns += [(2 * T + 1) * D + D - 1, 3 * T * D + D // 2, D - 1, max(L - 2, 0), 1, 0]
    return sorted(set(ns))


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("D,L", CASES)
def test_pairs_are_every_dth_output_of_the_shifted_filter(D, L, flip):
    """One call per length on a fresh tail, then a second short call on the tail the first one left: pairs and tail
    against the full-rate filter bit for bit (as values), and against the restatement in double."""
    c = lowpass_like_taps(L, 100 * D + L)
    zoom, fir = fsea.Zoom(c, D, 128), fsea.Fir(c)
    rng = np.random.default_rng(1000 * D + L + flip)
    for n in lengths(D, L):
        iq = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        more = rng.integers(0, 256, 2 * (3 * D + 1), dtype=np.uint8)
        zoom.reset()
        fir.reset()
        assert zoom.out_pairs(n) == n // D and zoom.out_rows(n) == (0 if n // D < 128 else (n // D - 128) // 128 + 1)
        _, got = zoom.run(iq, CPS, PHASE0, OFFSET, flip=bool(flip), pairs=True)
        full = fir.run_u8_shifted(iq, CPS, PHASE0, OFFSET, flip=bool(flip))
        assert got.shape == (n // D,) and np.array_equal(got, full[::D][:n // D]), (D, L, n, flip)
        tail = None
        if n:                                    # (the restatement's np.convolve takes no empty call)
            want, tail = zoom_reference(iq, flip, CPS, PHASE0, c, D, offset=OFFSET)
            check(got, want, (D, L, n, flip))
        # the tail the call left is the filter's: the next call continues both
        _, got = zoom.run(more, CPS, PHASE0, OFFSET + n, flip=bool(flip), pairs=True)
        full = fir.run_u8_shifted(more, CPS, PHASE0, OFFSET + n, flip=bool(flip))
        assert np.array_equal(got, full[::D][:(3 * D + 1) // D]), (D, L, n, flip, "second call")
        check(got, zoom_reference(more, flip, CPS, PHASE0, c, D, tail, offset=OFFSET + n)[0], (D, L, n, flip, "second call"))
    zoom.close()
    fir.close()


@pytest.mark.parametrize("D,L", [(16, 97), (25, 41), (64, 512)])
def test_a_stream_cut_at_multiples_of_d_is_the_one_call_result(D, L):
    c = lowpass_like_taps(L, 7 * D + L)
    cuts = [D * 1000, D * 37, D * (2 * T + 5)]
    n = sum(cuts)
    iq = np.random.default_rng(D * L).integers(0, 256, 2 * n, dtype=np.uint8)
    zoom = fsea.Zoom(c, D, 128, 64)
    rows, want = zoom.run(iq, CPS, PHASE0, OFFSET, flip=True, pairs=True)
    check(want, zoom_reference(iq, 1, CPS, PHASE0, c, D, offset=OFFSET)[0], (D, L))
    zoom.reset()
    got, pos = [], 0
    for k in cuts:
        got.append(zoom.run(iq[2 * pos:2 * (pos + k)], CPS, PHASE0, OFFSET + pos, flip=True, pairs=True)[1])
        pos += k
    assert np.array_equal(bits(np.concatenate(got)), bits(want))
    again = zoom.run(iq, CPS, PHASE0, OFFSET, flip=True, pairs=True)      # not reset: the tail of the stream's end
    assert not np.array_equal(again[1][:4], want[:4])
    zoom.reset()
    again = zoom.run(iq, CPS, PHASE0, OFFSET, flip=True, pairs=True)      # reset: the first result
    assert np.array_equal(bits(again[1]), bits(want)) and np.array_equal(again[0], rows)
    zoom.close()


def _rows_case(n_fft, hop, mode, window=None):
    D, L = 4, 41
    c = random_taps(L, n_fft + hop)
    n = (5 * n_fft + 3) * D + 1
    iq = np.random.default_rng(n_fft + hop + mode).integers(0, 256, 2 * n, dtype=np.uint8)
    zoom, plan = fsea.Zoom(c, D, n_fft, hop, mode), fsea.Plan(n_fft, hop, mode)
    if window is not None:
        zoom.set_window(window)
        plan.set_window(window)
    rows, pairs = zoom.run(iq, CPS, PHASE0, OFFSET, flip=True, pairs=True)
    n_rows = (n // D - n_fft) // hop + 1
    assert rows.shape == (n_rows, n_fft) and zoom.row_bytes == plan.row_bytes
    want = plan.exec_host_f64(pairs.view(np.float32).astype(np.float64), n_rows)
    assert np.array_equal(rows.view(np.uint8), want.view(np.uint8)), (n_fft, hop, mode)
    zoom.close()
    plan.close()
    # the same rows from the restatement in double: frame r is x[r hop : r hop + N] (-1)^n, weighted
    x = zoom_reference(iq, 1, CPS, PHASE0, c, D, offset=OFFSET)[0]
    w = np.ones(n_fft) if window is None else fsea.window(window, n_fft).astype(np.float64)
    sign = 1.0 - 2.0 * (np.arange(n_fft) % 2)
    spectra = np.stack([np.fft.fft(x[r * hop:r * hop + n_fft] * sign * w) for r in range(n_rows)])
    return rows, spectra


@pytest.mark.parametrize("mode", [fsea.MODE_MAG_F32, fsea.MODE_DB10_U8, fsea.MODE_COMPLEX_F32])
@pytest.mark.parametrize("hop_div", [1, 2, 4])
@pytest.mark.parametrize("n_fft", [128, 1024])
def test_rows_are_the_plans_rows_on_the_pairs(n_fft, hop_div, mode):
    rows, spectra = _rows_case(n_fft, n_fft // hop_div, mode)
    if mode == fsea.MODE_COMPLEX_F32:
        rel = float(np.linalg.norm(rows - spectra) / np.linalg.norm(spectra))
        print("N %d hop N/%d COMPLEX: relative L2 %.3e" % (n_fft, hop_div, rel))
        assert rel <= 2e-6, rel
    else:
        want = parity.rows_of_spectra(spectra, mode)
        dev = np.abs(rows.astype(np.float64) - want)
        print("N %d hop N/%d mode %d: max deviation %.3e (rows up to %.3e)" % (n_fft, hop_div, mode, dev.max(), want.max()))


@pytest.mark.parametrize("n_fft,hop", [(50, 50), (6, 3)])
def test_rows_of_a_byte_count_that_is_no_multiple_of_16_with_pairs(n_fft, hop):
    """5 rows of 50 bytes and 10 rows of 6 bytes on Bluestein plans, the pairs asked for: the rows do not end at a 16-byte
    boundary of the host form's staging, and the pairs that follow them come back from where they were put -- the rows
    recomputed from pairs read at a wrong offset would differ (_rows_case's bit identity)."""
    rows, _ = _rows_case(n_fft, hop, fsea.MODE_DB10_U8)
    assert rows.dtype == np.uint8 and rows.nbytes % 16 != 0, rows.shape


def test_rows_with_a_hann_window():
    rows, spectra = _rows_case(1024, 512, fsea.MODE_COMPLEX_F32, "hann")
    rel = float(np.linalg.norm(rows - spectra) / np.linalg.norm(spectra))
    print("Hann, N 1024 hop 512 COMPLEX: relative L2 %.3e" % rel)
    assert rel <= 2e-6, rel


def two_tones(n, rate=10e6, centre=1.25e6, apart=20e3, amp=40.0, sigma=20.0, seed=7):
    """Raw int8 IQ bytes: two tones `apart` Hz apart around `centre`, amplitude 40 each, over Gaussian noise sigma 20."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    s = amp * (np.exp(2j * np.pi * (centre - apart / 2) * t) + np.exp(2j * np.pi * (centre + apart / 2) * t))
    iq = np.empty(2 * n)
    iq[0::2] = s.real + rng.normal(0, sigma, n)
    iq[1::2] = s.imag + rng.normal(0, sigma, n)
    return np.clip(np.rint(iq), -128, 127).astype(np.int8).view(np.uint8)


def test_two_tones_20_khz_apart_share_a_bin_unzoomed_and_stand_four_bins_apart_zoomed():
    rate, centre, N, D = 10e6, 1.25e6, 128, 16
    raw = two_tones(1 << 18)
    # unzoomed: both in bin round(f N / rate) of the existing 128-point row, one peak
    cols = {N // 2 + int(round(f * N / rate)) for f in (centre - 10e3, centre + 10e3)}
    assert len(cols) == 1
    plan = fsea.Plan(N, N, fsea.MODE_MAG_F32)
    wide = plan.exec_host(raw, flip=True).astype(np.float64).mean(axis=0)
    plan.close()
    col = cols.pop()
    # the tones stand 0.13 bins either side of the bin's centre: with a rectangular frame the neighbours get at most
    # sinc(0.87) + sinc(1.13) = 0.26 of a tone, the bin itself 0.97 of both: a factor of 4.6 on average, 3 asserted
    assert int(np.argmax(wide)) == col and wide[col] > 3 * max(wide[col - 1], wide[col + 1])
    # zoomed on their midpoint: two peaks at N/2 +- round(10e3 D N / rate)
    zoom = fsea.Zoom(fsea.lowpass_taps(rate, 200e3, 97), D, N)
    rows, _ = zoom.run(raw, -centre / rate, flip=True)
    zoom.close()
    assert rows.shape == ((1 << 18) // D // N, N)
    m = rows.astype(np.float64).mean(axis=0)
    k = int(round(10e3 * D * N / rate))
    assert k == 2
    lo, hi = N // 2 - k, N // 2 + k
    assert set(np.argsort(m)[-2:]) == {lo, hi}, np.argsort(m)[-4:]
    between = m[N // 2 - 1]                      # the DC fix copies it into bin N/2
    assert m[lo] > 4 * between and m[hi] > 4 * between and m[lo] > 10 * np.median(m) and m[hi] > 10 * np.median(m)


def test_device_form_on_a_callers_stream_equals_the_host_form():
    D, L, N = 8, 97, 128
    c = random_taps(L, 5)
    n = (4 * N + 9) * D + 3
    iq = np.random.default_rng(3).integers(0, 256, 2 * n, dtype=np.uint8)
    zoom = fsea.Zoom(c, D, N, N // 2, fsea.MODE_MAG_F32)
    rows, pairs = zoom.run(iq, CPS, PHASE0, OFFSET, flip=True, pairs=True)
    sync = fsea.Plan(N)                          # fsea_stream_synchronize wants a plan for its device
    st = fsea.Stream()
    d_in = fsea.DeviceBuffer(iq.nbytes).upload(iq)
    d_rows, d_pairs = fsea.DeviceBuffer(rows.nbytes), fsea.DeviceBuffer(pairs.nbytes)
    for want_pairs in (True, False):
        zoom.reset()
        zoom.run_device(d_in.ptr.value, n, d_rows.ptr.value, CPS, PHASE0, OFFSET, flip=True,
                        d_pairs_ptr=d_pairs.ptr.value if want_pairs else None, stream=st)
        sync.synchronize(st)
        assert np.array_equal(bits(d_rows.download(np.float32, rows.shape)), bits(rows))
        if want_pairs:
            assert np.array_equal(bits(d_pairs.download(np.complex64, pairs.shape)), bits(pairs))
        d_rows.upload(np.zeros_like(rows))
    # what needs a real object to be refused: rows that have nowhere to go
    L_ = fsea.hip_lib()
    assert L_.fsea_zoom_run_device(zoom._p, d_in.ptr, n, 1, CPS, PHASE0, OFFSET, None, None, None) == FSEA_EINVAL
    assert L_.fsea_zoom_run_host(zoom._p, iq.ctypes.data, n, 1, CPS, PHASE0, OFFSET, None, None) == FSEA_EINVAL
    assert L_.fsea_zoom_run_host(zoom._p, iq.ctypes.data, D * (N - 1), 1, CPS, PHASE0, OFFSET, None, None) == 0   # no row
    # and what a plan refuses, the zoom refuses with the plan's status
    h = ctypes.c_void_p()
    plan_rc = [L_.fsea_plan_create(ctypes.byref(h), size, hop, mode, 0) for size, hop, mode in ((1, 8, 0), (128, 12, 0), (128, 128, 9))]
    zoom_rc = [L_.fsea_zoom_create(ctypes.byref(h), c.ctypes.data, L, D, size, hop, mode, 0)
               for size, hop, mode in ((1, 8, 0), (128, 12, 0), (128, 128, 9))]
    assert plan_rc == zoom_rc == [FSEA_EINVAL] * 3 and not h.value
    for b in (d_in, d_rows, d_pairs):
        b.free()
    st.close()
    sync.close()
    zoom.close()


def _history(L, z, n_fft, rows):
    buf = L.nrf_zoom_fft_get_buffer(z)
    assert buf.contents.length == n_fft * rows and buf.contents.channels == 1 and buf.contents.type == nrf.NUT_BUFFER_F64
    h = nrf.buffer_to_numpy(L, buf).reshape(rows, n_fft)
    L.nut_buffer_free(buf)
    return h


def test_host_block_scrolls_the_zoom_rows_into_its_history(golden_all):
    L = nrf.nrf_lib()
    rate, offset, D, N, H = 10000000, -1250000, 16, 128, 512
    block = np.ascontiguousarray(golden_all["block__raw"] ^ 0x80)
    n = block.size // 2
    z = L.nrf_zoom_fft_new(rate, offset, D, 200000, 97, N, H)
    zoom = fsea.Zoom(fsea.lowpass_taps(rate, 200000, 97), D, N)
    assert not _history(L, z, N, H).any()
    want = np.zeros((H, N))
    for k in range(3):
        buf = L.nut_buffer_new_u8(n, 2, block.ctypes.data)
        L.nrf_zoom_fft_process(z, buf)
        L.nut_buffer_free(buf)
        rows, _ = zoom.run(block, offset / rate, 0.0, k * n)
        assert rows.shape == (64, N)                                         # 131072 / 16 / 128: gapless
        want = np.concatenate([rows[::-1].astype(np.float64), want])[:H]    # newest first
        assert np.array_equal(_history(L, z, N, H), want), k
    # another centre: the phase and the filter start again, the history stays
    L.nrf_zoom_fft_set_freq_offset(z, 300000)
    zoom.reset()
    buf = L.nut_buffer_new_u8(n, 2, block.ctypes.data)
    L.nrf_zoom_fft_process(z, buf)
    L.nut_buffer_free(buf)
    rows, _ = zoom.run(block, 300000 / rate, 0.0, 0)
    want = np.concatenate([rows[::-1].astype(np.float64), want])[:H]
    assert np.array_equal(_history(L, z, N, H), want)
    L.nrf_zoom_fft_free(z)
    zoom.close()
    # a history shorter than a block's rows keeps the newest
    z = L.nrf_zoom_fft_new(rate, 300000, D, 200000, 97, N, 10)
    buf = L.nut_buffer_new_u8(n, 2, block.ctypes.data)
    L.nrf_zoom_fft_process(z, buf)
    L.nut_buffer_free(buf)
    assert np.array_equal(_history(L, z, N, 10), rows[::-1][:10].astype(np.float64))
    L.nrf_zoom_fft_free(z)


def test_host_block_refuses_an_f64_buffer():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n"
            "z = L.nrf_zoom_fft_new(10000000, 0, 16, 200000, 97, 128, 8)\n"
            "L.nrf_zoom_fft_process(z, L.nut_buffer_new_f64(4096, 2, None))\n"
            "print('returned')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF zoom FFT fatal error" in r.stderr and "F64" in r.stderr


def test_tool_writes_the_zoom_rows_and_prints_the_bin_width(tmp_path):
    from PIL import Image
    raw = two_tones(1 << 18)
    raw.tofile(tmp_path / "tones.raw")
    out = tmp_path / "zoom.png"
    r = subprocess.run([os.path.join(BIN, "fsea-zoom-fft"), str(tmp_path / "tones.raw"), "--rate", "10000000", "--offset",
                        "-1250000", "--decimation", "16", "--cutoff", "200000", "--taps", "97", "--fft", "128", "--out",
                        str(out)], capture_output=True, text=True, check=True, timeout=300)
    zoom = fsea.Zoom(fsea.lowpass_taps(10e6, 200e3, 97), 16, 128, 128, fsea.MODE_DB10_U8)
    rows, _ = zoom.run(raw, -1250000 / 10000000, flip=True)
    zoom.close()
    with Image.open(out) as im:
        got = np.array(im)
    assert got.dtype == np.uint8 and np.array_equal(got, rows)
    assert "rows %d" % rows.shape[0] in r.stdout and "bin width 4882.8125" in r.stdout
