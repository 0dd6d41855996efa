"""CPU tier: the frequency-shifted FIR filter and the IQ chain without a GPU -- the argument checks of
fsea_fir_u8_shifted_* and fsea_chain_* (before any device work), the fatal-error convention of nrf_iq_chain_new, the shipped
fsea_shift_fir_u8 kernel's resource usage, and the numpy restatement the GPU tests compare with (closed-form phase in
double, then tests/test_fir_host.py's fir_reference) against the reference's own recorded dvbt.lua chain
(tests/golden/iq_filter_golden.npz: dvbt__out)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests.conftest import ROOT
from tests.test_fir_host import GOLDEN, fir_reference
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1


def shifted_samples(u8, flip, delta, phase0, offset=0):
    """nrf_freq_shifter_process restated in double with a closed-form phase: sample m of the call, at stream position
    offset + m, is (u8 / 256) e^{2 pi i (phase0 + (offset + m) delta)} + 0.5 (1 + i)."""
    b = np.asarray(u8, dtype=np.uint8)
    b = b ^ 0x80 if flip else b
    x = b[0::2] / 256.0 + 1j * (b[1::2] / 256.0)
    turns = phase0 + (offset + np.arange(x.size, dtype=np.float64)) * delta
    turns -= np.floor(turns)
    return x * np.exp(2j * np.pi * turns) + (0.5 + 0.5j)


def shifted_fir_reference(u8, flip, delta, phase0, taps, tail=None, offset=0, n_zero=0):
    """The shifted filter in f64: the rotated block, followed by n_zero samples of plain 0.0 (the back half of the
    shifter's buffer), through fir_reference.  Returns (y, next tail)."""
    x = np.concatenate([shifted_samples(u8, flip, delta, phase0, offset), np.zeros(n_zero, dtype=np.complex128)])
    return fir_reference(x, taps, tail)


def test_restatement_reproduces_the_references_dvbt_chain():
    """Three steps of lua/dvbt.lua's shifter -> filter(5e6, 60e3, 97) on the replay block as the reference itself computed
    them: the phase runs on over the steps, every step filters N rotated pairs and N zero pairs.  1e-9: the closed-form
    phase differs from the reference's recurrence by the recurrence's drift, under 5e-12 over these three blocks."""
    with np.load(GOLDEN) as z:
        gold = {k: z[k] for k in z.files}
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        block = z["block__raw"] ^ 0x80
    n = block.size // 2
    delta = float(gold["dvbt__shift"]) / 5e6
    c = gold["taps__5000000_60000_97"]
    idx, tail = gold["dvbt__index"], None
    for step in range(3):
        y, tail = shifted_fir_reference(block, 0, delta, 0.0, c, tail, offset=step * n, n_zero=n)
        assert y.size == 2 * n
        want = gold["dvbt__out"][step]
        dev = float(np.max(np.abs(y[idx] - (want[:, 0] + 1j * want[:, 1]))))
        print("step %d: max deviation %.3e" % (step, dev))
        assert dev < 1e-9, (step, dev)
    # the check has teeth: a wrong sign, a missing phase carry or a missing offset are all far outside
    y, _ = shifted_fir_reference(block, 0, -delta, 0.0, c, None, n_zero=n)
    want = gold["dvbt__out"][0]
    assert np.max(np.abs(y[idx] - (want[:, 0] + 1j * want[:, 1]))) > 1e-3


def test_shifted_fir_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert L.fsea_fir_u8_shifted_host(None, p, 8, 0, 0.01, 0.0, 0, p) == FSEA_EINVAL
    assert L.fsea_fir_u8_shifted_device(None, p, 8, 0, 0.01, 0.0, 0, p, None) == FSEA_EINVAL
    # a fake object pointer: the remaining checks run before the object is touched
    fake = ctypes.create_string_buffer(4096)
    f = ctypes.cast(fake, ctypes.c_void_p)
    for cps, ph in ((np.nan, 0.0), (np.inf, 0.0), (0.01, np.nan), (0.01, -np.inf), (2.0 ** 21, 0.0)):
        assert L.fsea_fir_u8_shifted_host(f, p, 8, 0, cps, ph, 0, p) == FSEA_EINVAL, (cps, ph)
        assert L.fsea_fir_u8_shifted_device(f, p, 8, 0, cps, ph, 0, p, None) == FSEA_EINVAL, (cps, ph)
    assert b"cycles_per_sample" in L.fsea_last_error_string()
    assert L.fsea_fir_u8_shifted_host(f, p, 8, 0, 0.01, 0.0, (1 << 52) + 1, p) == FSEA_EINVAL
    assert L.fsea_fir_u8_shifted_device(f, p, 8, 0, 0.01, 0.0, (1 << 52) - 3, p, None) == FSEA_EINVAL
    assert L.fsea_fir_u8_shifted_device(f, p, (1 << 40) + 1, 0, 0.01, 0.0, 0, p, None) == FSEA_EINVAL
    assert L.fsea_fir_u8_shifted_device(f, None, 8, 0, 0.01, 0.0, 0, p, None) == FSEA_EINVAL
    assert L.fsea_fir_u8_shifted_device(f, p, 8, 0, 0.01, 0.0, 0, None, None) == FSEA_EINVAL
    assert L.fsea_fir_u8_shifted_device(f, p + 4, 8, 0, 0.01, 0.0, 0, p, None) == FSEA_EINVAL
    assert b"aligned" in L.fsea_last_error_string()
    assert L.fsea_fir_u8_shifted_host(f, None, 8, 0, 0.01, 0.0, 0, p) == FSEA_EINVAL
    assert L.fsea_fir_u8_shifted_host(f, p, 8, 0, 0.01, 0.0, 0, None) == FSEA_EINVAL


def test_chain_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    c = ctypes.c_void_p()
    taps = np.ones(fsea.FIR_MAX_TAPS + 1)
    for n in (0, -3, fsea.FIR_MAX_TAPS + 1):
        assert L.fsea_chain_create(ctypes.byref(c), taps.ctypes.data, n, 0) == FSEA_EINVAL, n
        assert not c.value
    assert L.fsea_chain_create(ctypes.byref(c), None, 21, 0) == FSEA_EINVAL
    assert L.fsea_chain_create(None, taps.ctypes.data, 21, 0) == FSEA_EINVAL
    bad = np.ones(21)
    bad[3] = np.inf
    assert L.fsea_chain_create(ctypes.byref(c), bad.ctypes.data, 21, 0) == FSEA_EINVAL
    assert b"not finite" in L.fsea_last_error_string()
    buf = np.zeros(64, np.uint8)
    assert L.fsea_chain_run_host(None, buf.ctypes.data, 8, None, None) == FSEA_EINVAL
    assert L.fsea_chain_run_f64_host(None, buf.ctypes.data, 2, None) == FSEA_EINVAL
    assert L.fsea_chain_fetch_host(None, None) == FSEA_EINVAL
    assert L.fsea_chain_run_device(None, buf.ctypes.data, 8, 1, None, None, None) == FSEA_EINVAL
    assert L.fsea_chain_reset(None) == FSEA_EINVAL and L.fsea_chain_destroy(None) == 0 and L.fsea_chain_n_pairs(None) == 0
    fake = ctypes.create_string_buffer(4096)
    f = ctypes.cast(fake, ctypes.c_void_p)
    p = buf.ctypes.data
    st = fsea.Chain.stage(n_zero=8)                                         # zero samples without a shift
    assert L.fsea_chain_run_host(f, p, 8, ctypes.byref(st), None) == FSEA_EINVAL
    assert L.fsea_chain_run_host(f, None, 8, None, None) == FSEA_EINVAL
    out = fsea.ChainOutputs(None, p, 0, 0, None)                              # size_multiplier 0
    assert L.fsea_chain_run_host(f, p, 8, None, ctypes.byref(out)) == FSEA_EINVAL
    out = fsea.ChainOutputs(None, p, 17, 0, None)
    assert L.fsea_chain_run_host(f, p, 8, None, ctypes.byref(out)) == FSEA_EINVAL
    out = fsea.ChainOutputs(None, p, 1, 9, None)                              # more line points than pairs
    assert L.fsea_chain_run_host(f, p, 8, None, ctypes.byref(out)) == FSEA_EINVAL
    assert L.fsea_chain_run_device(f, p, 8, -1, None, None, None) == FSEA_EINVAL
    st = fsea.Chain.stage(cycles_per_sample=0.01, n_zero=6)                 # frames with zeros: n a multiple of 8
    assert L.fsea_chain_run_device(f, p, 12, 2, ctypes.byref(st), None, None) == FSEA_EINVAL
    out = fsea.ChainOutputs(p + 8, None, 1, 0, None)                          # misaligned device output
    assert L.fsea_chain_run_device(f, p, 8, 1, None, ctypes.byref(out), None) == FSEA_EINVAL
    assert L.fsea_chain_run_device(f, (1 << 33), (1 << 31) + 1, 1, None, None, None) == FSEA_EINVAL


@pytest.mark.parametrize("length", [0, -1, fsea.FIR_MAX_TAPS + 1])
def test_iq_chain_with_a_bad_kernel_length_exits(length):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "nrf.nrf_lib().nrf_iq_chain_new(5000000, 200000, %d)\n"
            "print('returned')\n") % (ROOT, length)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "kernel length %d" % length in r.stderr


def test_chain_is_an_addition_in_the_full_host_library_only():
    names = [n for n in nrf.NRF_ADDITIONS if n.startswith("nrf_iq_chain_")]
    assert len(names) == 7 and not set(names) & set(nrf.NRF_EXPORTS)
    pkg = os.path.join(ROOT, "frequensea_amd")
    full = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pkg, "libfsea_nrf.so")], capture_output=True,
                          text=True, check=True).stdout.split()
    assert set(names) <= set(full)
    fft_only = os.path.join(pkg, "libfsea_nrf_fft.so")
    if os.path.exists(fft_only):
        syms = subprocess.run(["nm", "-D", "--defined-only", fft_only], capture_output=True, text=True, check=True).stdout
        assert "nrf_iq_chain" not in syms


def test_shipped_library_has_the_shifted_fir_kernel_without_spills():
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    k = ks["fsea_shift_fir_u8"]
    assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]                       # eight waves per SIMD by registers
    assert k[".group_segment_fixed_size"] == ks["fsea_fir_u8"][".group_segment_fixed_size"] <= 32 * 1024
