"""GPU tier: the streaming complex FIR filter (fsea_fir_*, kernels fsea_fir_u8 / fsea_fir_f64) and the nrf_iq_filter block
on top of it, against the f64 numpy restatement (tests/test_fir_host.py: fir_reference, np.convolve per channel) and the
reference's own outputs (tests/golden/iq_filter_golden.npz).

Tolerance: max |delta| <= 1e-5 and relative L2 <= 1e-6.  The kernel rounds each tap to f32 and accumulates in f32 with one
FMA per tap (u = 2^-24 per rounding); u8 / 256 is exact in f32, f64 inputs are rounded once.  With |x| <= 1.5 (the
inputs: [0, 1) from u8, [-0.5, 1.5] from the shifter) and sum|c| = S < 2:
  - tap rounding: sum |c_k - fl(c_k)| |x| <= u S 1.5 <= 1.8e-7;
  - input rounding (f64 only): u S 1.5, the same;
  - accumulation: each of the L FMAs rounds a partial sum bounded by S 1.5, so at worst L u S 1.5 -- 1.7e-5 at L = 97,
    S = 2 -- but those roundings are independent and of zero mean: their sum has a standard deviation of about
    sqrt(L / 3) u S 1.5 <= 2.3e-6 even at L = 512, so 1e-5 is more than four standard deviations of a single output's
    error at the cap and far more at the scenes' lengths (the low-pass designs have S ~ 1.1, the test taps S = 1).
  - relative L2: the errors of different outputs are independent, so the ratio is ~ sqrt(L / 3) u S 1.5 / rms(y) with
    rms(y) >= ~0.3 for these inputs (offset-binary bytes: mean 0.5 on both channels): ~1e-7, well under 1e-6."""
import ctypes
import threading
import time

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests.test_fir_host import GOLDEN, fir_reference

pytestmark = pytest.mark.gpu

MAX_ABS, MAX_REL = 1e-5, 1e-6
LENGTHS = [1, 2, 21, 50, 51, 97, fsea.FIR_MAX_TAPS]
COUNTS = [1, 7, "L-2", 2047, 2048, 2049, 131072, (1 << 22) + 13]


def check(got, want, what=""):
    got = np.asarray(got, dtype=np.complex128)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return
    err = np.abs(got - want)
    rel = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    assert err.max() <= MAX_ABS and rel <= MAX_REL, (what, float(err.max()), float(rel))


def random_taps(L, seed):
    """Non-symmetric taps with sum |c| = 1."""
    c = np.random.default_rng(seed).standard_normal(L)
    return c / np.abs(c).sum()


def u8_to_complex(iq, flip):
    b = iq ^ 0x80 if flip else iq
    return b[0::2] / 256.0 + 1j * (b[1::2] / 256.0)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("flip", [0, 1])
def test_sizes_against_the_restatement(L, flip):
    c = random_taps(L, L)
    fir = fsea.Fir(c)
    rng = np.random.default_rng(1000 + L)
    for n in COUNTS:
        n = L - 2 if n == "L-2" else n
        if n < 1:
            continue
        fir.reset()
        iq = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        got = fir.run_u8(iq, flip=bool(flip))
        want, _ = fir_reference(u8_to_complex(iq, flip), c)
        check(got, want, (L, n, flip))
    fir.close()


@pytest.mark.parametrize("L", [21, 97, fsea.FIR_MAX_TAPS])
def test_f64_input(L):
    c = random_taps(L, 7 * L)
    fir = fsea.Fir(c)
    rng = np.random.default_rng(L)
    x = rng.uniform(-0.5, 1.5, 40000) + 1j * rng.uniform(-0.5, 1.5, 40000)
    check(fir.run_f64(x), fir_reference(x, c)[0], L)
    fir.close()


@pytest.mark.parametrize("L", [2, 51, 97, fsea.FIR_MAX_TAPS])
def test_calls_of_random_lengths_continue_one_stream(L):
    """A stream cut into calls of random lengths (1 and shorter than the tail among them) gives what one call over the whole
    stream gives -- bit for bit: every output sums the same f32 products in the same order; reset() starts afresh."""
    c = random_taps(L, 3 * L)
    rng = np.random.default_rng(L)
    cuts = [1, L - 2 if L > 2 else 1, 3, 5000, 1, 2048, 17, 70000, 1, L // 2 + 1, 33333]
    iq = rng.integers(0, 256, 2 * sum(cuts), dtype=np.uint8)
    whole = fsea.Fir(c)
    want = whole.run_u8(iq, flip=True)
    check(want, fir_reference(u8_to_complex(iq, 1), c)[0], L)
    parts = fsea.Fir(c)
    got, pos = [], 0
    for n in cuts:
        got.append(parts.run_u8(iq[2 * pos:2 * (pos + n)], flip=True))
        pos += n
    assert np.array_equal(np.concatenate(got), want)
    parts.reset()
    assert np.array_equal(parts.run_u8(iq, flip=True), want)          # after reset: a fresh object's result
    whole.close()
    parts.close()


def _replay_device(L, tmp_path, raw):
    path = tmp_path / "block.raw"
    raw.tofile(path)
    dev = L.nrf_device_new(100.0, str(path).encode())   # the file-replay device, sample rate 5e6
    L.nrf_device_set_paused(dev, 1)
    return dev


@pytest.mark.parametrize("cutoff,length", [(200e3, 51), (60e3, 97)])
def test_replay_device_through_nrf_iq_filter(gold, tmp_path, cutoff, length):
    with np.load(GOLDEN.replace("iq_filter_golden", "rfdata_all_golden")) as z:
        raw = z["block__raw"]
    L = nrf.nrf_lib()
    dev = _replay_device(L, tmp_path, raw)
    flt = L.nrf_iq_filter_new(5000000, int(cutoff), length)
    c = gold["taps__5000000_%d_%d" % (cutoff, length)][:length]
    idx, tail = gold["iq__index"], None
    for step in range(3):
        L.nrf_device_step(dev)
        time.sleep(0.06)
        buf = L.nrf_device_get_samples_buffer(dev)
        L.nrf_iq_filter_process(flt, buf)
        out = L.nrf_iq_filter_get_buffer(flt)
        assert out.contents.type == nrf.NUT_BUFFER_F64 and out.contents.channels == 2
        v = nrf.buffer_to_numpy(L, out)
        y = v[0::2] + 1j * v[1::2]
        want, tail = fir_reference(u8_to_complex(raw, 1), c, tail)
        check(y, want, (cutoff, length, step))
        ref = gold["iq__%d_%d__out" % (cutoff, length)][step]
        check(y[idx], ref[:, 0] + 1j * ref[:, 1], ("reference", cutoff, length, step))
        L.nut_buffer_free(out)
        L.nut_buffer_free(buf)
    L.nrf_iq_filter_free(flt)
    L.nrf_device_free(dev)


def test_dvbt_chain_shifter_into_filter(gold, tmp_path):
    """lua/dvbt.lua: nrf_freq_shifter -> nrf_iq_filter(5e6, 60e3, 97); the shifter's buffer has 2N pairs (back half zero)
    and the filter follows buffer->length: 2N pairs in, 2N out."""
    with np.load(GOLDEN.replace("iq_filter_golden", "rfdata_all_golden")) as z:
        raw = z["block__raw"]
    L = nrf.nrf_lib()
    dev = _replay_device(L, tmp_path, raw)
    shifter = L.nrf_freq_shifter_new(int(gold["dvbt__shift"]), 5000000)
    flt = L.nrf_iq_filter_new(5000000, 60000, 97)
    c = gold["taps__5000000_60000_97"]
    idx, tail = gold["dvbt__index"], None
    for step in range(3):
        L.nrf_device_step(dev)
        time.sleep(0.06)
        buf = L.nrf_device_get_samples_buffer(dev)
        L.nrf_freq_shifter_process(shifter, buf)
        sb = L.nrf_freq_shifter_get_buffer(shifter)
        L.nrf_iq_filter_process(flt, sb)
        out = L.nrf_iq_filter_get_buffer(flt)
        assert out.contents.length == raw.size
        v = nrf.buffer_to_numpy(L, out)
        y = v[0::2] + 1j * v[1::2]
        s = nrf.buffer_to_numpy(L, sb)
        want, tail = fir_reference(s[0::2] + 1j * s[1::2], c, tail)
        check(y, want, ("dvbt", step))
        ref = gold["dvbt__out"][step]
        check(y[idx], ref[:, 0] + 1j * ref[:, 1], ("dvbt reference", step))
        for b in (out, sb, buf):
            L.nut_buffer_free(b)
    L.nrf_iq_filter_free(flt)
    L.nrf_freq_shifter_free(shifter)
    L.nrf_device_free(dev)


def test_u8_and_f64_buffers_in_one_filter_and_empty_get_buffer():
    L = nrf.nrf_lib()
    flt = L.nrf_iq_filter_new(5000000, 200000, 51)
    out = L.nrf_iq_filter_get_buffer(flt)
    assert out.contents.length == 0 and out.contents.channels == 2 and out.contents.type == nrf.NUT_BUFFER_F64
    L.nut_buffer_free(out)
    c = fsea.lowpass_taps(5e6, 200e3, 51)
    rng = np.random.default_rng(5)
    tail, got, want = None, [], []
    for step, kind in enumerate(["u8", "f64", "u8", "f64", "u8"]):
        n = [3000, 20, 10, 4096, 1][step]
        if kind == "u8":
            data = rng.integers(0, 256, 2 * n, dtype=np.uint8)
            buf = L.nut_buffer_new_u8(n, 2, data.ctypes.data)
            x = u8_to_complex(data, 0)
        else:
            data = rng.uniform(-0.5, 1.5, 2 * n)
            buf = L.nut_buffer_new_f64(n, 2, data.ctypes.data)
            x = data[0::2] + 1j * data[1::2]
        L.nrf_iq_filter_process(flt, buf)
        out = L.nrf_iq_filter_get_buffer(flt)
        assert out.contents.length == n
        v = nrf.buffer_to_numpy(L, out)
        got.append(v[0::2] + 1j * v[1::2])
        y, tail = fir_reference(x, c, tail)
        want.append(y)
        L.nut_buffer_free(out)
        L.nut_buffer_free(buf)
    check(np.concatenate(got), np.concatenate(want), "mixed")
    L.nrf_iq_filter_free(flt)


def test_two_filters_on_two_threads_keep_their_own_state():
    cs = [random_taps(97, 1), random_taps(51, 2)]
    rng = np.random.default_rng(9)
    streams = [rng.integers(0, 256, 2 * 300000, dtype=np.uint8) for _ in cs]
    results = [None, None]

    def run(k):
        fir = fsea.Fir(cs[k])
        parts, pos = [], 0
        for n in [1000, 7, 50000, 20, 123456, 1, 125516]:
            parts.append(fir.run_u8(streams[k][2 * pos:2 * (pos + n)]))
            pos += n
        results[k] = np.concatenate(parts)
        fir.close()

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k in range(2):
        check(results[k], fir_reference(u8_to_complex(streams[k], 0), cs[k])[0], k)


def test_device_form_is_deterministic():
    """Two identical launches of the device-resident form write bit-identical output (the store-hazard class of bug shows
    up as run-to-run differences)."""
    L = fsea.hip_lib()
    n = (1 << 22) + 13
    c = random_taps(97, 97)
    iq = np.random.default_rng(3).integers(0, 256, 2 * n, dtype=np.uint8)
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    fsea._check(L.fsea_device_alloc(0, iq.nbytes, ctypes.byref(d_in)))
    fsea._check(L.fsea_device_alloc(0, 8 * n, ctypes.byref(d_out)))
    fsea._check(L.fsea_copy_to_device(0, d_in, iq.ctypes.data, iq.nbytes))
    outs = []
    for _ in range(2):
        fir = fsea.Fir(c)
        fir.run_device(d_in.value, n, d_out.value, flip=True)
        y = np.empty(n, dtype=np.complex64)
        fsea._check(L.fsea_copy_to_host(0, y.ctypes.data, d_out, 8 * n))
        fir.close()
        outs.append(y)
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    check(outs[0], fir_reference(u8_to_complex(iq, 1), c)[0], "device")
    fsea._check(L.fsea_device_free(0, d_in))
    fsea._check(L.fsea_device_free(0, d_out))
