"""CPU tier: the polyphase filter bank without a GPU -- the two numpy restatements of tests/pfb_ref.py against each other
(rotated polyphase frames + centred DFT = the direct per-channel form), the prototype design, the leakage statement the
bank exists for, the argument checks of fsea_pfb_* (before any device work), the fatal-error convention of nrf_pfb_fft_new
and the shipped kernels' resource usage."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import parity, pfb_ref
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
IDENTITY_CASES = [(8, 4, 8), (8, 3, 2), (6, 4, 3), (12, 4, 3), (32, 8, 16), (50, 4, 25)]   # (M, P, D)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("M,P,D", IDENTITY_CASES)
def test_rotated_polyphase_frames_and_a_centred_dft_are_the_direct_form(M, P, D):
    """Two calls: the first from a zero tail and s0 = 0 with a length that is no multiple of D, the second on the tail and
    the s0 it left.  1e-12: both sides are f64 sums of at most 128 terms of size <= 1."""
    rng = np.random.default_rng(M * P + D)
    c = rng.standard_normal(M * P)
    tail, s0 = None, 0
    for n in (7 * D + D // 2 + 1, 5 * D):
        iq = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        frames, t1 = pfb_ref.pfb_frames_reference(iq, 1, c, M, D, tail, s0)
        want, t2 = pfb_ref.pfb_direct(iq, 1, c, M, D, tail, s0)
        assert frames.shape == (n // D, M) and np.array_equal(t1, t2) and t1.size == M * P - 1
        rel = _rel(pfb_ref.rows_of(frames), want)
        print("M %d P %d D %d s0 %d: relative %.3e" % (M, P, D, s0, rel))
        assert rel <= 1e-12, (M, P, D, s0, rel)
        tail, s0 = t1, s0 + n


def test_the_identity_check_has_teeth():
    """No rotation at q = 2, a rotation by t D without s0 on a second call, taps read branch-major: each far outside."""
    M, P, D = 8, 4, 4
    rng = np.random.default_rng(5)
    c = rng.standard_normal(M * P)
    iq = rng.integers(0, 256, 2 * (9 * D + 1), dtype=np.uint8)
    more = rng.integers(0, 256, 2 * 6 * D, dtype=np.uint8)
    want, tail = pfb_ref.pfb_direct(iq, 0, c, M, D)
    assert _rel(pfb_ref.rows_of(pfb_ref.pfb_frames_reference(iq, 0, c, M, D)[0]), want) <= 1e-12
    assert _rel(pfb_ref.rows_of(pfb_ref.pfb_frames_reference(iq, 0, c, M, D, variant="no_rotation")[0]), want) > 1e-3
    assert _rel(pfb_ref.rows_of(pfb_ref.pfb_frames_reference(iq, 0, c, M, D, variant="branch_major")[0]), want) > 1e-3
    s0 = 9 * D + 1
    want2, _ = pfb_ref.pfb_direct(more, 0, c, M, D, tail, s0)
    assert _rel(pfb_ref.rows_of(pfb_ref.pfb_frames_reference(more, 0, c, M, D, tail, s0)[0]), want2) <= 1e-12
    assert _rel(pfb_ref.rows_of(pfb_ref.pfb_frames_reference(more, 0, c, M, D, tail, s0, variant="no_s0")[0]), want2) > 1e-3


@pytest.mark.parametrize("M", [32, 128, 1024])
@pytest.mark.parametrize("P", [2, 3, 4, 8, 16])
def test_prototype_is_the_scaled_lowpass_and_its_branches_are_small(M, P):
    """Bit for bit M x lowpass_taps(2 M, 1, M P); every branch has sum |c| < 2, the premise of the GPU tier's 1e-5 / 1e-6."""
    c = fsea.pfb_prototype(M, P)
    assert c.shape == (M * P,) and np.array_equal(c, M * fsea.lowpass_taps(2 * M, 1, M * P))
    s = np.abs(c.reshape(P, M)).sum(axis=0)
    print("M %d P %d: branch sum |c| in [%.3f, %.3f], sum c %.4f" % (M, P, s.min(), s.max(), c.sum()))
    assert s.max() < 2.0


def test_the_bank_does_not_leak_where_a_rectangular_frame_does():
    """A tone half-way between channels 74 and 75 of 128: its leakage three channels away and further, over the peak, in
    MAG rows (the oracle's: the DC column patched, as the plan's)."""
    M, P, frames = 128, 8, 72
    raw = pfb_ref.tone_bytes(M, frames)
    bank = pfb_ref.rows_of(pfb_ref.pfb_frames_reference(raw, 1, fsea.pfb_prototype(M, P), M, M)[0])
    top, ratio = pfb_ref.leakage(parity.rows_of_spectra(bank[8:], fsea.MODE_MAG_F32).mean(axis=0))
    print("bank: largest columns %s, leakage %.3e" % (sorted(top), ratio))
    assert top == {74, 75} and ratio <= 1e-2
    rect = pfb_ref.rows_of(pfb_ref.u8_to_complex(raw, 1).reshape(frames, M))
    top, ratio = pfb_ref.leakage(parity.rows_of_spectra(rect[8:], fsea.MODE_MAG_F32).mean(axis=0))
    print("rectangular: largest columns %s, leakage %.3e" % (sorted(top), ratio))
    assert top == {74, 75} and ratio >= 0.1


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()
    assert int(re.search(r"#define FSEA_PFB_MAX_CHANNELS (\d+)", text).group(1)) == fsea.PFB_MAX_CHANNELS == 16384
    assert int(re.search(r"#define FSEA_PFB_MAX_BRANCH_TAPS (\d+)", text).group(1)) == fsea.PFB_MAX_BRANCH_TAPS == 16


def test_pfb_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    b = ctypes.c_void_p()
    taps = np.ones(64 * 17)
    t = taps.ctypes.data

    def create(channels, branch_taps, q, taps_ptr=t, out=ctypes.byref(b)):
        rc = L.fsea_pfb_create(out, taps_ptr, channels, branch_taps, q, 0, 0)
        assert not b.value
        return rc

    for m in (0, -2, 1, 7, 33, fsea.PFB_MAX_CHANNELS + 2):                  # out of range, odd
        assert create(m, 4, 1) == FSEA_EINVAL, m
        assert b"channels" in L.fsea_last_error_string()
    for p in (0, -1, 17):
        assert create(64, p, 1) == FSEA_EINVAL, p
        assert b"branch_taps" in L.fsea_last_error_string()
    for m, q in ((64, 0), (64, 3), (64, 8), (64, -1), (6, 4), (50, 4)):       # not 1, 2 or 4; no divisor of the channels
        assert create(m, 4, q) == FSEA_EINVAL, (m, q)
        assert b"oversampling" in L.fsea_last_error_string()
    assert create(64, 4, 1, taps_ptr=None) == FSEA_EINVAL and b"taps is NULL" in L.fsea_last_error_string()
    assert L.fsea_pfb_create(None, t, 64, 4, 1, 0, 0) == FSEA_EINVAL
    bad = np.ones(64 * 4)
    bad[200] = np.inf
    assert create(64, 4, 1, taps_ptr=bad.ctypes.data) == FSEA_EINVAL and b"tap 200 is not finite" in L.fsea_last_error_string()

    out = np.zeros(64 * 17)
    for m, p in ((7, 4), (0, 4), (fsea.PFB_MAX_CHANNELS + 2, 4), (64, 0), (64, 17)):
        assert L.fsea_pfb_prototype(m, p, out.ctypes.data) == FSEA_EINVAL, (m, p)
    assert L.fsea_pfb_prototype(64, 4, None) == FSEA_EINVAL

    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert L.fsea_pfb_run_host(None, p, 8, 0, p, None, None) == FSEA_EINVAL
    assert L.fsea_pfb_run_device(None, p, 8, 0, p, None, None, None) == FSEA_EINVAL
    assert L.fsea_pfb_reset(None) == FSEA_EINVAL and L.fsea_pfb_destroy(None) == 0
    assert L.fsea_pfb_out_frames(None, 64) == 0 and L.fsea_pfb_row_bytes(None) == 0
    # a fake object pointer (all zero: mode FSEA_MODE_MAG_F32): the remaining checks run before the object is used
    fake = ctypes.create_string_buffer(4096)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert L.fsea_pfb_run_host(f, p, 8, 0, p, None, p) == FSEA_EINVAL                 # a series outside COMPLEX mode
    assert b"FSEA_MODE_COMPLEX_F32" in L.fsea_last_error_string()
    assert L.fsea_pfb_run_device(f, p, 8, 0, p, None, p, None) == FSEA_EINVAL
    assert b"FSEA_MODE_COMPLEX_F32" in L.fsea_last_error_string()
    assert L.fsea_pfb_run_host(f, p, (1 << 31) + 1, 0, p, None, None) == FSEA_EINVAL
    assert L.fsea_pfb_run_device(f, p, (1 << 31) + 1, 0, p, None, None, None) == FSEA_EINVAL
    assert b"too large" in L.fsea_last_error_string()
    assert L.fsea_pfb_run_host(f, None, 8, 0, p, None, None) == FSEA_EINVAL
    assert L.fsea_pfb_run_device(f, None, 8, 0, p, None, None, None) == FSEA_EINVAL
    assert b"NULL" in L.fsea_last_error_string()
    for d_iq, d_rows, d_frames in ((p + 4, p, None), (p, p + 8, None), (p, p, p + 2)):
        assert L.fsea_pfb_run_device(f, d_iq, 8, 0, d_rows, d_frames, None, None) == FSEA_EINVAL
        assert b"aligned" in L.fsea_last_error_string()


def _child(body, env=""):
    code = ("import os, sys; sys.path.insert(0, %r)\n%s"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n%s\nprint('returned')\n") % (ROOT, env, body)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("fft_size", [0, 1, 127, fsea.PFB_MAX_CHANNELS + 2])
def test_pfb_fft_with_a_bad_fft_size_exits(fft_size):
    r = _child("L.nrf_pfb_fft_new(%d, 512, 8)" % fft_size)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PFB FFT fatal error: fft size %d" % fft_size in r.stderr


@pytest.mark.parametrize("branch_taps", [0, -1, fsea.PFB_MAX_BRANCH_TAPS + 1])
def test_pfb_fft_with_bad_branch_taps_exits(branch_taps):
    r = _child("L.nrf_pfb_fft_new(128, 512, %d)" % branch_taps)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PFB FFT fatal error: branch taps %d" % branch_taps in r.stderr


def test_pfb_fft_with_a_bad_history_size_exits():
    r = _child("L.nrf_pfb_fft_new(128, 0, 8)")
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PFB FFT fatal error: history size 0" in r.stderr


def test_pfb_fft_backend_failure_exits():
    """A device that does not exist, with or without a GPU in the machine: the backend's status and text, then exit."""
    r = _child("L.nrf_pfb_fft_new(128, 512, 8)", env="os.environ['NRF_FFT_DEVICE'] = '4096'\n")
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PFB FFT fatal error: fsea_pfb_create failed" in r.stderr


def test_pfb_fft_is_an_addition_in_the_full_host_library_only():
    names = [n for n in nrf.NRF_ADDITIONS if n.startswith("nrf_pfb_fft_")]
    assert len(names) == 4 and not set(names) & set(nrf.NRF_EXPORTS)
    pkg = os.path.join(ROOT, "frequensea_amd")
    full = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pkg, "libfsea_nrf.so")], capture_output=True,
                          text=True, check=True).stdout.split()
    assert set(names) <= set(full)
    fft_only = os.path.join(pkg, "libfsea_nrf_fft.so")
    if os.path.exists(fft_only):
        syms = subprocess.run(["nm", "-D", "--defined-only", fft_only], capture_output=True, text=True, check=True).stdout
        assert "nrf_pfb_fft" not in syms


def test_shipped_library_has_the_bank_kernels_within_their_budget():
    """The three LDS sizes of fsea_pfb_frames_u8 and the transpose: wave64, 256 lanes, no scratch, no spills, at most 80 KiB
    of static LDS (two workgroups on a CU's 160 KiB at the largest) and 128 VGPRs (four waves per SIMD)."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    for name, lds in (("fsea_pfb_frames_u8_s", 20 * 1024), ("fsea_pfb_frames_u8_m", 40 * 1024), ("fsea_pfb_frames_u8", 80 * 1024),
                      ("fsea_pfb_transpose", 32 * 33 * 8)):
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] == lds <= 80 * 1024, (name, k[".group_segment_fixed_size"])
    # every (M, P, q) has a tile whose image fits the largest kernel's LDS
    for M in (2, 6, 32, 64, 100, 128, 256, 258, 1024, 16384):
        for P in range(1, 17):
            for q in (1, 2, 4):
                if M % q:
                    continue
                C, T = pfb_ref.tile_shape(M, P, q)
                assert T >= 1 and (T + (2 * ((P + 1) // 2) - 1) * q) * C * 8 <= 80 * 1024, (M, P, q, C, T)
