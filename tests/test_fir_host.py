"""CPU tier: the IQ low-pass filter's host side -- the reference's tap design and per-sample FIR filter (bit for bit against
tests/golden/iq_filter_golden.npz, which tests/golden/make_iq_filter_golden.py records from the reference's own src/nrf.c),
the argument checks of fsea_fir_* (before any device work), the fatal-error convention of nrf_iq_filter_new, the numpy
restatement the GPU tests compare with, and the shipped fsea_fir_* kernels' resource usage."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

GOLDEN = os.path.join(ROOT, "tests", "golden", "iq_filter_golden.npz")
SCENE_PAIRS = [(10e3, 21), (60e3, 97), (80e3, 43), (100e3, 23), (200e3, 51), (200e3, 97), (100e3, 51)]
QUIRK_LENGTHS = [1, 2, 50]
FSEA_EINVAL = -1


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fir_reference(x, c, tail=None):
    """The filter restated in numpy, f64: y[i] = sum_k c[k] x_ext[i + k], x_ext = tail ++ x, per channel.  Returns
    (y, next tail)."""
    c = np.asarray(c, dtype=np.float64)
    L = c.size
    tail = np.zeros(L - 1, dtype=np.complex128) if tail is None else tail
    x_ext = np.concatenate([tail, np.asarray(x, dtype=np.complex128)])
    y = np.convolve(x_ext.real, c[::-1], "valid") + 1j * np.convolve(x_ext.imag, c[::-1], "valid")
    return y, x_ext[x_ext.size - (L - 1):]


def test_header_cap_matches_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()
    assert int(re.search(r"#define FSEA_FIR_MAX_TAPS (\d+)", text).group(1)) == fsea.FIR_MAX_TAPS >= 255


@pytest.mark.parametrize("rate", [5000000, 10000000])
def test_lowpass_taps_are_the_references_bit_for_bit(gold, rate):
    L = nrf.nrf_lib()
    for cutoff, length in SCENE_PAIRS + [(200e3, n) for n in QUIRK_LENGTHS]:
        want = gold["taps__%d_%d_%d" % (rate, cutoff, length)]
        m = length + (length + 1) % 2
        assert want.size == m
        # the C ABI: the first `length` of the m designed taps (what the reference's filter uses)
        got = fsea.lowpass_taps(rate, cutoff, length)
        assert got.size == length and np.array_equal(got, want[:length]), (rate, cutoff, length)
        # the reference's own entry point in libfsea_nrf.so: all m taps
        p = L.nrf_fir_get_low_pass_coefficients(rate, int(cutoff), length)
        got = np.ctypeslib.as_array(p, shape=(m,)).copy()
        ctypes.CDLL(None).free(ctypes.cast(p, ctypes.c_void_p))
        assert np.array_equal(got, want), (rate, cutoff, length)
    # the quirk itself: an even length uses a prefix of a longer design, which is not symmetric
    t = fsea.lowpass_taps(rate, 200e3, 50)
    assert t.size == 50 and not np.array_equal(t, t[::-1]) and np.array_equal(t, fsea.lowpass_taps(rate, 200e3, 51)[:50])


def test_fir_filter_pull_api_is_the_references_bit_for_bit(gold):
    L = nrf.nrf_lib()
    x, loads, want = gold["fir__in"], gold["fir__loads"], gold["fir__out"]
    f = L.nrf_fir_filter_new(5000000, 100000, 51)
    assert f.contents.length == 51 and f.contents.offset == 50 and f.contents.center == 25
    got, pos = [], 0
    for n in loads:                                         # 4096, 1000, 20 (< L - 1), 3000
        chunk = np.ascontiguousarray(x[pos:pos + n])
        pos += n
        L.nrf_fir_filter_load(f, chunk.ctypes.data, int(n))
        assert f.contents.samples_length == n + 50
        got.extend(L.nrf_fir_filter_get(f, i) for i in range(n))
    L.nrf_fir_filter_free(f)
    assert np.array_equal(np.array(got), want)


def test_numpy_restatement_matches_the_reference_filter(gold):
    """The f64 restatement the GPU tests use, against the reference's nrf_iq_filter on the replay device's block (three
    steps: the tail carries over) and on the dvbt.lua chain's 2N-pair shifter buffer."""
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        block = z["block__raw"] ^ 0x80
    x = block[0::2] / 256.0 + 1j * (block[1::2] / 256.0)
    idx = gold["iq__index"]
    for cutoff, length in ((200e3, 51), (60e3, 97)):
        c = gold["taps__5000000_%d_%d" % (cutoff, length)][:length]
        tail = None
        for step in range(3):
            y, tail = fir_reference(x, c, tail)
            want = gold["iq__%d_%d__out" % (cutoff, length)][step]
            assert np.max(np.abs(y[idx] - (want[:, 0] + 1j * want[:, 1]))) < 1e-12, (cutoff, length, step)
    # dvbt.lua: this library's nrf_freq_shifter (host, double) in front, its 2N-pair buffer filtered whole
    L = nrf.nrf_lib()
    shifter = L.nrf_freq_shifter_new(int(gold["dvbt__shift"]), 5000000)
    c = gold["taps__5000000_60000_97"]
    idx, tail = gold["dvbt__index"], None
    for step in range(3):
        buf = L.nut_buffer_new_u8(block.size // 2, 2, np.ascontiguousarray(block).ctypes.data)
        L.nrf_freq_shifter_process(shifter, buf)
        sb = L.nrf_freq_shifter_get_buffer(shifter)
        v = nrf.buffer_to_numpy(L, sb)
        assert sb.contents.length == block.size and not v[block.size:].any()
        y, tail = fir_reference(v[0::2] + 1j * v[1::2], c, tail)
        want = gold["dvbt__out"][step]
        assert np.max(np.abs(y[idx] - (want[:, 0] + 1j * want[:, 1]))) < 1e-12, step
        L.nut_buffer_free(sb)
        L.nut_buffer_free(buf)
    L.nrf_freq_shifter_free(shifter)


def test_fir_create_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    f = ctypes.c_void_p()
    taps = np.ones(fsea.FIR_MAX_TAPS + 1)
    for n in (0, -3, fsea.FIR_MAX_TAPS + 1):
        assert L.fsea_fir_create(ctypes.byref(f), taps.ctypes.data, n, 0) == FSEA_EINVAL, n
        assert not f.value
    assert L.fsea_fir_create(ctypes.byref(f), None, 21, 0) == FSEA_EINVAL
    assert L.fsea_fir_create(None, taps.ctypes.data, 21, 0) == FSEA_EINVAL
    bad = np.ones(21)
    bad[7] = np.nan
    assert L.fsea_fir_create(ctypes.byref(f), bad.ctypes.data, 21, 0) == FSEA_EINVAL
    assert b"not finite" in L.fsea_last_error_string()
    out = np.zeros(16, np.float32)
    assert L.fsea_fir_u8_host(None, out.ctypes.data, 8, 0, out.ctypes.data) == FSEA_EINVAL
    assert L.fsea_fir_f64_host(None, out.ctypes.data, 8, out.ctypes.data) == FSEA_EINVAL
    assert L.fsea_fir_u8_device(None, out.ctypes.data, 8, 0, out.ctypes.data, None) == FSEA_EINVAL
    assert L.fsea_fir_reset(None) == FSEA_EINVAL and L.fsea_fir_destroy(None) == 0 and L.fsea_fir_n_taps(None) == 0
    t = np.zeros(4)
    assert L.fsea_fir_lowpass_taps(5e6, 200e3, 0, t.ctypes.data) == FSEA_EINVAL
    assert L.fsea_fir_lowpass_taps(0.0, 200e3, 4, t.ctypes.data) == FSEA_EINVAL
    assert L.fsea_fir_lowpass_taps(5e6, 200e3, 4, None) == FSEA_EINVAL


@pytest.mark.parametrize("length", [0, -1, fsea.FIR_MAX_TAPS + 1])
def test_iq_filter_with_a_bad_kernel_length_exits(length):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "nrf.nrf_lib().nrf_iq_filter_new(5000000, 200000, %d)\n"
            "print('returned')\n") % (ROOT, length)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "kernel length %d" % length in r.stderr


def test_shipped_library_has_the_fir_kernels_without_spills():
    if not os.path.exists(LIB):
        pytest.skip("libfsea_hip.so not built")
    ks = _kernels(LIB)
    fir = sorted(k for k in ks if k.startswith("fsea_fir"))
    assert fir == ["fsea_fir_f64", "fsea_fir_u8"]
    for name in fir:
        k = ks[name]
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 64, (name, k[".vgpr_count"])          # eight waves per SIMD by registers
        assert k[".group_segment_fixed_size"] <= 32 * 1024, name          # five workgroups per CU by LDS
