"""CPU tier of the signal capture: fsea_detect_finish / fsea_detect_moments against nrf_signal_detector_process (pinned to
the reference's recorded values by tests/test_iq_draw_host.py) and against exact rational arithmetic, fsea_capture_segment
against the literal state machine of tests/capture_ref.py, and the argument checks of fsea_detect_*, fsea_capture_* and
fsea-signal-capture (before any device work).  Nothing here needs a GPU."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import capture_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-signal-capture")
EINVAL, ENODEVICE = -1, -2
U = 2.0 ** -53
PREFIXES = [2, 30, 4098, 16384, 262144]
DIVISORS = [1, 2, 4, 8, 64]


@pytest.fixture(scope="module")
def block():
    """The replay device's block as nrf_device_get_samples_buffer hands it out (offset binary)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        return np.ascontiguousarray(z["block__raw"] ^ 0x80)


def reference_detector(a):
    """nrf_signal_detector_process on a uint8 array: (mean, standard_deviation)."""
    L = nrf.nrf_lib()
    a = np.ascontiguousarray(a, dtype=np.uint8)
    buf = L.nut_buffer_new_u8(a.size // 2, 2, a.ctypes.data)
    det = L.nrf_signal_detector_new()
    L.nrf_signal_detector_process(det, buf)
    got = det.contents.mean, det.contents.standard_deviation
    L.nrf_signal_detector_free(det)
    L.nut_buffer_free(buf)
    return got


def sd_bound(n):
    """The reference's sequential sum of n positive terms is within about (n + 1) 2^-53 of exact, the root halves that; 16
    more cover the finish, the division and the root."""
    return (n / 2 + 16) * U


def moments(s, n):
    a = np.array(s, dtype=np.uint64)
    mean, diffs = ctypes.c_double(), ctypes.c_double()
    assert fsea.hip_lib().fsea_detect_moments(a.ctypes.data, n, ctypes.byref(mean), ctypes.byref(diffs)) == 0
    return mean.value, diffs.value


@pytest.mark.parametrize("divisor", DIVISORS)
def test_finish_equals_the_reference_detector(block, divisor):
    quiet = R.scale_about_128(block, divisor)
    for n in PREFIXES:
        a = quiet[:n]
        mean, sd = fsea.detect_finish(R.sums(a), n)
        want_mean, want_sd = reference_detector(a)
        rel = abs(sd - want_sd) / want_sd
        print("divisor %d n %d: mean %r sd %r reference sd %r rel %.3g bound %.3g" % (divisor, n, mean, sd, want_sd, rel,
                                                                                     sd_bound(n)))
        assert mean == want_mean, (divisor, n)
        assert rel <= sd_bound(n), (divisor, n, rel)


def test_finish_meets_the_recorded_values_of_the_reference(block):
    with np.load(os.path.join(ROOT, "tests", "golden", "iq_draw_golden.npz")) as z:
        want = z["detector__block"]
    mean, sd = fsea.detect_finish(R.sums(block), block.size)
    assert abs(want[0] - 0.49049276) < 1e-8 and want[1] == 140.89637750973804
    assert mean == want[0]
    assert abs(sd - want[1]) / want[1] <= sd_bound(block.size)


def adversarial(n, rng):
    v = int(rng.integers(3, 252))
    w = int(rng.integers(0, 256))
    one = np.full(n, v, np.uint8)
    one[int(rng.integers(0, n))] = w
    alt = np.full(n, v, np.uint8)
    alt[1::2] = w
    return {
        "uniform": rng.integers(0, 256, n, dtype=np.uint8),
        "v or v + 1": (v + rng.integers(0, 2, n)).astype(np.uint8),
        "all v but one": one,
        "v +- 3": (v + rng.integers(-3, 4, n)).astype(np.uint8),
        "evens v, odds w": alt,
        "all v": np.full(n, v, np.uint8),
    }


@pytest.mark.parametrize("n", [2, 4, 6, 30, 258, 4098, 65536])
def test_moments_against_exact_rational_arithmetic(n):
    rng = np.random.default_rng(n)
    for name, a in adversarial(n, rng).items():
        s = R.sums(a)
        mean, diffs = moments(s, n)
        assert mean == (s[0] / 256.0) / n * 2, name
        exact = R.exact_diffs_total(s, n, mean)
        if exact == 0:
            assert diffs == 0.0, (name, n)
            continue
        rel = abs(Fraction(diffs) - exact) / exact
        print("n %d %s: relative error %.3g x 2^-53" % (n, name, float(rel) / U))
        assert rel <= 8 * U, (name, n, float(rel) / U)
        _, sd = fsea.detect_finish(s, n)
        assert sd == math.sqrt(diffs / mean), (name, n)


def test_all_zero_bytes_give_nan_as_the_reference():
    for n in (2, 30, 4098):
        mean, sd = fsea.detect_finish((0, 0, 0), n)
        want_mean, want_sd = reference_detector(np.zeros(n, np.uint8))
        assert mean == 0.0 == want_mean and math.isnan(sd) and math.isnan(want_sd)


def runs_as_bursts(runs):
    return [list(range(first, first + count)) for first, count, _, _ in runs]


NAN = float("nan")
SEGMENT_CASES = {
    "no burst": [10.0, 99.0, 0.0, 50.0],
    "a burst at block 0": [140.0, 141.0, 70.0, 70.0],
    "a burst at the last block": [70.0, 70.0, 140.0],
    "two bursts and one quiet block between": [70.0, 140.0, 140.0, 70.0, 140.0, 70.0],
    "NaN entries": [NAN, 140.0, NAN, 140.0, 140.0, NAN, NAN],
    "sd equal to the threshold": [100.0, 100.0000001, 100.0, 99.9999999],
    "all above": [101.0, 102.0, 103.0],
    "one block": [140.0],
}


@pytest.mark.parametrize("name", sorted(SEGMENT_CASES))
def test_segment_is_the_scenes_state_machine(name):
    sd = SEGMENT_CASES[name]
    for capturing in (False, True):
        labels, bursts, state = R.scene(sd, 100.0, R.CAPTURING if capturing else R.DETECTING)
        runs = fsea.capture_segment(sd, 100.0, capturing)
        assert runs_as_bursts(runs) == bursts, (name, capturing)
        assert [r[2] for r in runs] == [capturing and k == 0 for k in range(len(runs))]
        assert [r[3] for r in runs] == [state == R.CAPTURING and k == len(runs) - 1 for k in range(len(runs))]
        assert len(runs) <= len(sd) // 2 + 1
    if name == "two bursts and one quiet block between":
        assert R.scene(sd, 100.0)[0] == ["idle", "start", "captured", "end", "start", "end"]
    if name == "sd equal to the threshold":
        assert fsea.capture_segment(sd, 100.0) == [(1, 1, False, False)]
    if name == "no burst":
        assert fsea.capture_segment(sd, 100.0) == [] and fsea.capture_segment(sd, NAN) == []


def test_segment_of_random_statistics_and_two_scans():
    rng = np.random.default_rng(5)
    sd = rng.choice([70.0, 140.0, NAN, 100.0], 400)
    labels, bursts, state = R.scene(sd, 100.0)
    assert runs_as_bursts(fsea.capture_segment(sd, 100.0)) == bursts
    # cut anywhere: the second scan continues the first one's open burst
    for cut in (1, 57, 200, 399):
        first = fsea.capture_segment(sd[:cut], 100.0)
        still_open = bool(first) and first[-1][3]
        second = fsea.capture_segment(sd[cut:], 100.0, still_open)
        joined = runs_as_bursts(first)
        rest = [[b + cut for b in run] for run in runs_as_bursts(second)]
        if still_open:
            joined[-1] += rest.pop(0)
        assert joined + rest == bursts, cut


def test_detect_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    d = ctypes.c_void_p()
    assert L.fsea_detect_create(None, 0) == EINVAL
    assert L.fsea_detect_destroy(None) == 0
    buf = np.zeros(1 << 12, np.uint8)
    out = np.zeros(64, np.float64)
    p, o = buf.ctypes.data, out.ctypes.data
    assert L.fsea_detect_u8_host(None, p, 16, 1, 0, o, o) == EINVAL
    assert L.fsea_detect_u8_device(None, p, 16, 1, 0, o, None) == EINVAL
    # a non-NULL object that is never dereferenced: every check below fails before the object or a device is used
    fake = ctypes.c_void_p(p)
    a16 = (p + 15) & ~15
    for block_bytes in (0, 1, 3, 4097, (1 << 31) + 2):
        assert L.fsea_detect_u8_host(fake, p, block_bytes, 1, 0, o, o) == EINVAL, block_bytes
        assert L.fsea_detect_u8_device(fake, a16, block_bytes, 1, 0, o, None) == EINVAL, block_bytes
    assert b"block_bytes" in L.fsea_last_error_string()
    assert L.fsea_detect_u8_host(fake, p, 16, 0, 0, o, o) == EINVAL                          # n_blocks
    assert L.fsea_detect_u8_device(fake, a16, 16, 0, 0, o, None) == EINVAL
    assert L.fsea_detect_u8_host(fake, p, 1 << 30, 1 << 11, 0, o, o) == EINVAL               # more than 2^40 bytes
    assert L.fsea_detect_u8_host(fake, None, 16, 1, 0, o, o) == EINVAL
    assert L.fsea_detect_u8_host(fake, p, 16, 1, 0, None, o) == EINVAL
    assert L.fsea_detect_u8_device(fake, None, 16, 1, 0, o, None) == EINVAL
    assert L.fsea_detect_u8_device(fake, a16, 16, 1, 0, None, None) == EINVAL
    assert L.fsea_detect_u8_device(fake, a16 + 2, 16, 1, 0, (o + 15) & ~15, None) == EINVAL  # misaligned pointers
    assert L.fsea_detect_u8_device(fake, a16, 16, 1, 0, ((o + 15) & ~15) + 8, None) == EINVAL
    assert b"aligned" in L.fsea_last_error_string()
    m, s = ctypes.c_double(), ctypes.c_double()
    sums = np.array([1, 2, 3], np.uint64)
    for n in (0, 1, 3, (1 << 31) + 2):
        assert L.fsea_detect_finish(sums.ctypes.data, n, ctypes.byref(m), ctypes.byref(s)) == EINVAL, n
    assert L.fsea_detect_finish(None, 2, ctypes.byref(m), ctypes.byref(s)) == EINVAL
    assert L.fsea_detect_finish(sums.ctypes.data, 2, None, ctypes.byref(s)) == EINVAL
    assert L.fsea_detect_finish(sums.ctypes.data, 2, ctypes.byref(m), None) == EINVAL
    assert L.fsea_detect_finish(np.array([256, 2, 3], np.uint64).ctypes.data, 2, ctypes.byref(m), ctypes.byref(s)) == EINVAL
    assert not d.value and not buf.any() and not out.any()


def test_capture_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    c = ctypes.c_void_p()
    taps = fsea.lowpass_taps(5e6, 200e3, 97)
    assert L.fsea_capture_create(None, taps.ctypes.data, 97, 0) == EINVAL
    for n_taps in (0, -1, fsea.FIR_MAX_TAPS + 1):                                          # bad taps come before the device
        assert L.fsea_capture_create(ctypes.byref(c), taps.ctypes.data, n_taps, 0) == EINVAL and not c.value
    assert L.fsea_capture_create(ctypes.byref(c), None, 97, 0) == EINVAL
    bad = taps.copy()
    bad[5] = np.inf
    assert L.fsea_capture_create(ctypes.byref(c), bad.ctypes.data, 97, 0) == EINVAL and not c.value
    assert L.fsea_capture_destroy(None) == 0 and L.fsea_capture_reset(None) == EINVAL
    assert L.fsea_capture_n_bursts(None) == 0 and L.fsea_capture_n_blocks(None) == 0
    buf = np.zeros(1 << 12, np.uint8)
    p = buf.ctypes.data
    a16 = (p + 15) & ~15
    m, s = ctypes.c_double(), ctypes.c_double()
    assert L.fsea_capture_scan_host(None, p, 16, 1, 0, 100.0) == EINVAL
    assert L.fsea_capture_scan_device(None, a16, 16, 1, 0, 100.0, None) == EINVAL
    assert L.fsea_capture_stats(None, 0, ctypes.byref(m), ctypes.byref(s)) == EINVAL
    assert L.fsea_capture_burst(None, 0, ctypes.byref(fsea.CaptureBurstInfo())) == EINVAL
    assert L.fsea_capture_burst_pairs_host(None, 0, p) == EINVAL
    assert L.fsea_capture_burst_lines_host(None, 0, 1, 0, p) == EINVAL
    assert L.fsea_capture_burst_lines_device(None, 0, 1, 0, a16, None) == EINVAL
    fake = ctypes.c_void_p(p)
    for block_bytes in (0, 2, 8, 30, 4098, 16392, (1 << 31) + 16):                          # multiples of 16 only
        assert L.fsea_capture_scan_host(fake, p, block_bytes, 1, 0, 100.0) == EINVAL, block_bytes
        assert L.fsea_capture_scan_device(fake, a16, block_bytes, 1, 0, 100.0, None) == EINVAL, block_bytes
    assert b"block_bytes" in L.fsea_last_error_string()
    assert L.fsea_capture_scan_host(fake, p, 16, 0, 0, 100.0) == EINVAL
    assert L.fsea_capture_scan_host(fake, None, 16, 1, 0, 100.0) == EINVAL
    assert L.fsea_capture_scan_device(fake, None, 16, 1, 0, 100.0, None) == EINVAL
    assert L.fsea_capture_scan_device(fake, a16 + 8, 16, 1, 0, 100.0, None) == EINVAL
    for mult in (0, -1, fsea.IQ_MAX_MULTIPLIER + 1):
        assert L.fsea_capture_burst_lines_host(fake, 0, mult, 0, p) == EINVAL
        assert L.fsea_capture_burst_lines_device(fake, 0, mult, 0, a16, None) == EINVAL
    assert L.fsea_capture_burst_lines_host(fake, 0, 1, 0, None) == EINVAL
    assert L.fsea_capture_burst_lines_device(fake, 0, 1, 0, a16 + 4, None) == EINVAL
    assert L.fsea_capture_burst_pairs_host(fake, 0, None) == EINVAL
    n = ctypes.c_size_t(7)
    runs = (fsea.CaptureRun * 4)()
    assert L.fsea_capture_segment(None, 3, 100.0, 0, runs, ctypes.byref(n)) == EINVAL and n.value == 0
    assert L.fsea_capture_segment(buf.ctypes.data, 3, 100.0, 0, None, ctypes.byref(n)) == EINVAL
    assert L.fsea_capture_segment(buf.ctypes.data, 3, 100.0, 0, runs, None) == EINVAL
    assert not buf.any()


def test_create_without_a_gpu_is_enodevice():
    L = fsea.hip_lib()
    d, c = ctypes.c_void_p(), ctypes.c_void_p()
    taps = fsea.lowpass_taps(5e6, 200e3, 97)
    rd = L.fsea_detect_create(ctypes.byref(d), 0)
    rc = L.fsea_capture_create(ctypes.byref(c), taps.ctypes.data, 97, 0)
    if fsea.device_count() > 0:
        assert rd == 0 and d.value and L.fsea_detect_destroy(d) == 0
        assert rc == 0 and c.value and L.fsea_capture_destroy(c) == 0
        return
    assert rd == ENODEVICE and not d.value and rc == ENODEVICE and not c.value
    with pytest.raises(fsea.FseaError):
        fsea.Detect()
    with pytest.raises(fsea.FseaError):
        fsea.Capture(taps)


def test_tool_is_built_and_rejects_bad_arguments(tmp_path):
    if not os.path.exists(TOOL):
        pytest.fail("fsea-signal-capture is not built: run __graft_entry__.build()")
    rec = tmp_path / "recording.raw"
    np.zeros(4096, np.uint8).tofile(str(rec))
    out = tmp_path / "out"
    out.mkdir()
    common = [TOOL, "--out-dir", str(out)]
    for args in (["--block-bytes", "0"], ["--block-bytes", "30"], ["--block-bytes", "4098"], ["--block-bytes", "-16"],
                 ["--threshold", "nan"], ["--sample-rate", "0"], ["--taps", "0"], ["--taps", "513"], ["--multiplier", "0"],
                 ["--multiplier", "17"], ["--step", "0"], ["--step", "-0.5"], ["--step", "nan"], ["--step", "0.00001"], ["--step", "0.0001"],
                 ["--cutoff", "-1"], ["--cutoff", "2500001"],
                 ["--bogus"], ["--taps"]):
        r = subprocess.run(common + args + [str(rec)], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "fsea-signal-capture" in r.stderr, args
        assert "NRF" not in r.stderr and "fsea_capture_create" not in r.stderr, args    # refused before any device work
    r = subprocess.run(common, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no recording" in r.stderr
    r = subprocess.run(common + [str(rec), str(rec)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "usage" in r.stderr
    r = subprocess.run(common + [str(tmp_path / "nowhere.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cannot open recording" in r.stderr
    r = subprocess.run(common + ["--block-bytes", "8192", str(rec)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "less than one block" in r.stderr
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shader gain" in r.stdout and "alpha fade" in r.stdout and "out of scope" in r.stdout
    assert not list(out.iterdir())


def test_shipped_library_has_the_detector_kernels_without_spills():
    if not os.path.exists(LIB):
        pytest.fail("libfsea_hip.so is not built: run __graft_entry__.build()")
    ks = _kernels(LIB)
    names = sorted(k for k in ks if k.startswith("fsea_detect_"))
    assert names == ["fsea_detect_slices", "fsea_detect_waves"]
    for name in names:
        k = ks[name]
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 64, name     # a SIMD holds its eight waves: the stream hides its latency by occupancy
    assert ks["fsea_detect_waves"][".group_segment_fixed_size"] == 0


def test_exports_are_listed_once():
    names = [n for n in nrf.NRF_ADDITIONS if n.startswith("nrf_signal_capture_")]
    assert len(names) == 7 and not set(names) & set(nrf.NRF_EXPORTS)
    assert len([n for n in fsea.EXPORTS if n.startswith(("fsea_detect_", "fsea_capture_"))]) == 19
