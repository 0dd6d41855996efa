"""CPU tier: the zoom spectrum without a GPU -- the numpy restatement the GPU tests compare with (tests/test_iq_chain_host.py's
shifted filter, every D-th output) against the reference's own recorded nrf_freq_shifter -> nrf_downsampler chain
(tests/golden/zoom_golden.npz, written by tests/golden/make_zoom_golden.py), the argument checks of fsea_zoom_* (before any
device work), the fatal-error convention of nrf_zoom_fft_new, and the shipped fsea_shift_decim_u8 kernels' resource usage."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests.conftest import ROOT
from tests.test_iq_chain_host import shifted_fir_reference
from tests.test_shipped_artifacts import LIB, _kernels

GOLDEN = os.path.join(ROOT, "tests", "golden", "zoom_golden.npz")
RATE_PAIRS = [(5000000, 312500, 16), (5000000, 200000, 25), (3000000, 1000000, 3)]
LENGTHS = [41, 97]
FSEA_EINVAL = -1


def zoom_reference(u8, flip, delta, phase0, taps, D, tail=None, offset=0):
    """The decimating filter in f64: the rotated block through the full-rate filter (x_ext = tail ++ x), outputs 0, D, 2 D,
    ... of it, n // D of them; the tail is the full-rate filter's.  Returns (pairs, next tail)."""
    y, tail = shifted_fir_reference(u8, flip, delta, phase0, taps, tail, offset=offset)
    return y[::D][:y.size // D], tail


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def block():
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        return z["block__raw"] ^ 0x80


def _deviation(y, gold, tag, k):
    want = gold["%s__out%d" % (tag, k)]
    return float(np.max(np.abs(y[gold["%s__idx%d" % (tag, k)]] - (want[:, 0] + 1j * want[:, 1]))))


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("rin,rout,D", RATE_PAIRS)
def test_restatement_reproduces_the_references_shifter_and_downsampler(gold, block, rin, rout, D, length):
    """Three consecutive calls of nrf_freq_shifter_process -> nrf_downsampler_process (I and Q) on the replay block as the
    reference itself computed them: the phase and the filter's tail run on over the calls, the decimation restarts with
    every call (131072 is no multiple of 25 or 3).  1e-9: the closed-form phase against the reference's recurrence, the
    bound tests/test_iq_chain_host.py uses for the same difference."""
    tag = "zoom__%d_%d_%d" % (rin, rout, length)
    assert tuple(gold[tag + "__cfg"]) == (D, rout // 2, length)
    c = gold[tag + "__taps"]
    assert np.array_equal(c, fsea.lowpass_taps(rin, rout // 2, length))
    n = block.size // 2
    delta = float(gold["shift"]) / rin
    tail = None
    for k in range(3):
        y, tail = zoom_reference(block, 0, delta, 0.0, c, D, tail, offset=k * n)
        assert y.size == int(gold[tag + "__len"]) == n // D
        dev = _deviation(y, gold, tag, k)
        print("%s call %d: max deviation %.3e" % (tag, k, dev))
        assert dev < 1e-9, (tag, k, dev)


def test_the_check_against_the_reference_has_teeth(gold, block):
    """A wrong decimation, a wrong sign of the shift and a missing tail carry are each far outside 1e-9."""
    tag, D, rin = "zoom__5000000_312500_97", 16, 5000000
    c, n = gold[tag + "__taps"], block.size // 2
    delta = float(gold["shift"]) / rin
    y0, tail = zoom_reference(block, 0, delta, 0.0, c, D)
    assert _deviation(y0, gold, tag, 0) < 1e-9
    y, _ = zoom_reference(block, 0, delta, 0.0, c, D // 2)                               # a wrong D
    assert _deviation(y, gold, tag, 0) > 1e-3
    y, _ = zoom_reference(block, 0, -delta, 0.0, c, D)                                   # a wrong sign
    assert _deviation(y, gold, tag, 0) > 1e-3
    y, _ = zoom_reference(block, 0, delta, 0.0, c, D, None, offset=n)                    # the second call without its tail
    assert _deviation(y, gold, tag, 1) > 1e-3
    y, _ = zoom_reference(block, 0, delta, 0.0, c, D, tail, offset=n)                    # and with it
    assert _deviation(y, gold, tag, 1) < 1e-9


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()
    assert int(re.search(r"#define FSEA_ZOOM_MAX_DECIMATION (\d+)", text).group(1)) == fsea.ZOOM_MAX_DECIMATION == 64
    assert int(re.search(r"#define FSEA_ZOOM_TILE_OUTPUTS (\d+)", text).group(1)) == fsea.ZOOM_TILE_OUTPUTS


def test_zoom_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    z = ctypes.c_void_p()
    taps = np.ones(fsea.FIR_MAX_TAPS + 1)
    t = taps.ctypes.data
    for n in (0, -3, fsea.FIR_MAX_TAPS + 1):
        assert L.fsea_zoom_create(ctypes.byref(z), t, n, 4, 128, 128, 0, 0) == FSEA_EINVAL, n
        assert not z.value
    assert b"n_taps" in L.fsea_last_error_string()
    for d in (0, -1, fsea.ZOOM_MAX_DECIMATION + 1):
        assert L.fsea_zoom_create(ctypes.byref(z), t, 21, d, 128, 128, 0, 0) == FSEA_EINVAL, d
        assert not z.value
    assert b"decimation" in L.fsea_last_error_string()
    assert L.fsea_zoom_create(ctypes.byref(z), None, 21, 4, 128, 128, 0, 0) == FSEA_EINVAL
    assert L.fsea_zoom_create(None, t, 21, 4, 128, 128, 0, 0) == FSEA_EINVAL
    bad = np.ones(21)
    bad[3] = np.nan
    assert L.fsea_zoom_create(ctypes.byref(z), bad.ctypes.data, 21, 4, 128, 128, 0, 0) == FSEA_EINVAL
    assert b"not finite" in L.fsea_last_error_string()

    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert L.fsea_zoom_run_host(None, p, 8, 0, 0.01, 0.0, 0, p, None) == FSEA_EINVAL
    assert L.fsea_zoom_run_device(None, p, 8, 0, 0.01, 0.0, 0, p, None, None) == FSEA_EINVAL
    assert L.fsea_zoom_reset(None) == FSEA_EINVAL and L.fsea_zoom_set_window(None, p) == FSEA_EINVAL
    assert L.fsea_zoom_destroy(None) == 0
    assert L.fsea_zoom_out_pairs(None, 64) == 0 and L.fsea_zoom_out_rows(None, 64) == 0 and L.fsea_zoom_row_bytes(None) == 0
    # a fake object pointer: the remaining checks run before the object is touched
    fake = ctypes.create_string_buffer(4096)
    f = ctypes.cast(fake, ctypes.c_void_p)
    for cps, ph in ((np.nan, 0.0), (np.inf, 0.0), (0.01, np.nan), (0.01, -np.inf), (2.0 ** 21, 0.0)):
        assert L.fsea_zoom_run_host(f, p, 8, 0, cps, ph, 0, p, None) == FSEA_EINVAL, (cps, ph)
        assert L.fsea_zoom_run_device(f, p, 8, 0, cps, ph, 0, p, None, None) == FSEA_EINVAL, (cps, ph)
    assert b"cycles_per_sample" in L.fsea_last_error_string()
    assert L.fsea_zoom_run_host(f, p, 8, 0, 0.01, 0.0, (1 << 52) + 1, p, None) == FSEA_EINVAL
    assert L.fsea_zoom_run_device(f, p, 8, 0, 0.01, 0.0, (1 << 52) - 3, p, None, None) == FSEA_EINVAL
    assert L.fsea_zoom_run_device(f, p, (1 << 31) + 1, 0, 0.01, 0.0, 0, p, None, None) == FSEA_EINVAL
    assert L.fsea_zoom_run_host(f, None, 8, 0, 0.01, 0.0, 0, p, None) == FSEA_EINVAL
    assert L.fsea_zoom_run_device(f, None, 8, 0, 0.01, 0.0, 0, p, None, None) == FSEA_EINVAL
    assert b"NULL" in L.fsea_last_error_string()
    for d_iq, d_rows, d_pairs in ((p + 4, p, None), (p, p + 8, None), (p, p, p + 2)):
        assert L.fsea_zoom_run_device(f, d_iq, 8, 0, 0.01, 0.0, 0, d_rows, d_pairs, None) == FSEA_EINVAL
        assert b"aligned" in L.fsea_last_error_string()


def _child(body):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n%s\nprint('returned')\n") % (ROOT, body)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("length", [0, -1, fsea.FIR_MAX_TAPS + 1])
def test_zoom_fft_with_a_bad_kernel_length_exits(length):
    r = _child("L.nrf_zoom_fft_new(10000000, 0, 16, 300000, %d, 128, 512)" % length)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF zoom FFT fatal error: kernel length %d" % length in r.stderr


@pytest.mark.parametrize("decimation", [0, -2, fsea.ZOOM_MAX_DECIMATION + 1])
def test_zoom_fft_with_a_bad_decimation_exits(decimation):
    r = _child("L.nrf_zoom_fft_new(10000000, 0, %d, 300000, 97, 128, 512)" % decimation)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF zoom FFT fatal error: decimation %d" % decimation in r.stderr


def test_zoom_fft_backend_failure_exits():
    """A device that does not exist, with or without a GPU in the machine: the backend's status and text, then exit."""
    code = ("import os, sys; sys.path.insert(0, %r)\n"
            "os.environ['NRF_FFT_DEVICE'] = '4096'\n"
            "from frequensea_amd import nrf\n"
            "nrf.nrf_lib().nrf_zoom_fft_new(10000000, 0, 16, 300000, 97, 128, 512)\n"
            "print('returned')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF zoom FFT fatal error: fsea_zoom_create failed" in r.stderr


def test_zoom_fft_is_an_addition_in_the_full_host_library_only():
    names = [n for n in nrf.NRF_ADDITIONS if n.startswith("nrf_zoom_fft_")]
    assert len(names) == 5 and not set(names) & set(nrf.NRF_EXPORTS)
    pkg = os.path.join(ROOT, "frequensea_amd")
    full = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pkg, "libfsea_nrf.so")], capture_output=True,
                          text=True, check=True).stdout.split()
    assert set(names) <= set(full)
    fft_only = os.path.join(pkg, "libfsea_nrf_fft.so")
    if os.path.exists(fft_only):
        syms = subprocess.run(["nm", "-D", "--defined-only", fft_only], capture_output=True, text=True, check=True).stdout
        assert "nrf_zoom_fft" not in syms


def test_shipped_library_has_the_decimating_kernels_within_their_budget():
    """The three LDS sizes of fsea_shift_decim_u8: 256 lanes, no scratch, registers for eight waves per SIMD, and LDS for
    eight, four and two workgroups on a CU's 160 KiB (the largest holds D = 64, L = 512)."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    cu_lds = 160 * 1024
    for name, per_cu in (("fsea_shift_decim_u8_s", 8), ("fsea_shift_decim_u8_m", 4), ("fsea_shift_decim_u8", 2)):
        k = ks[name]
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 64, (name, k[".vgpr_count"])
        assert cu_lds // k[".group_segment_fixed_size"] == per_cu, (name, k[".group_segment_fixed_size"])
    # the largest image: D phases of ZOOM_TILE_OUTPUTS + ceil((L - 1) / D) columns (made odd), 8 bytes a sample
    D, taps = fsea.ZOOM_MAX_DECIMATION, fsea.FIR_MAX_TAPS
    need = D * ((fsea.ZOOM_TILE_OUTPUTS + (taps - 1 + D - 1) // D) | 1) * 8
    assert need <= ks["fsea_shift_decim_u8"][".group_segment_fixed_size"]
    assert not [k for k in ks if k.startswith("fsea_fft") and "decim" in k]
