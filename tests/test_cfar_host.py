"""CPU tier: the CFAR spectrum detector without a GPU -- the two numpy restatements of tests/cfar_ref.py against each other,
fsea_cfar_bands against bands_of, the argument checks of fsea_cfar_* (before any device work), the header's constants, the
fatal-error convention of nrf_spectrum_occupancy_*, the tool's usage message and the shipped kernels' resource usage."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import cfar_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-occupancy")


@pytest.mark.parametrize("width", [1, 2, 5, 17, 70])
def test_the_two_restatements_agree(width):
    rng = np.random.default_rng(width)
    for G in (0, 1, 3):
        for T in (1, 4, 40):
            for offset in (-5, 0, 20):
                for method in (R.CA, R.GO, R.SO):
                    rows = rng.integers(0, 256, (3, width), dtype=np.uint8)
                    rows[1] = rng.integers(100, 110, width)                     # a flat row: many near-ties
                    a, b = R.detect(rows, G, T, offset, method), R.detect_loops(rows, G, T, offset, method)
                    assert np.array_equal(a, b), (width, G, T, offset, method)
    rows = (rng.normal(-60, 8, (2, width))).astype(np.float32)
    rows[0, 0] = np.nan
    for method in (R.CA, R.GO, R.SO):
        assert np.array_equal(R.detect(rows, 1, 4, 3 * 64, method), R.detect_loops(rows, 1, 4, 3 * 64, method))


def test_the_restatements_f32_levels():
    v = np.array([0.0, 1.0, -1.0, 0.5 / 64, 1.5 / 64, 2.5 / 64, -0.5 / 64, -2.5 / 64, 16384.0, 16383.99, -16384.0, -16383.99,
                  np.inf, -np.inf, np.nan, 1e30, -1e30, 3e38], np.float32)
    assert R.levels_of_f32(v).tolist() == [0, 64, -64, 0, 2, 2, 0, -2, 1 << 20, 1048575, -(1 << 20), -1048575,
                                           1 << 20, -(1 << 20), -(1 << 20), 1 << 20, -(1 << 20), 1 << 20]
    assert R.levels_of(np.array([[0, 7, 255]], np.uint8)).tolist() == [[0, 7, 255]]


def test_a_carrier_one_can_read_off():
    """A flat row at 50 with one cell at 120: with (2, 4, 60) the cell is a hit (120 > 50 + 60) and no other cell is; the
    cells whose training window holds the carrier see a mean of (3 * 50 + 120) / 4 = 67.5 on that side."""
    row = np.full((1, 40), 50, np.uint8)
    row[0, 20] = 120
    for method in (R.CA, R.GO, R.SO):
        assert np.flatnonzero(R.detect(row, 2, 4, 60, method)[0]).tolist() == [20]
    # offset -10 under GO: every cell but those with the carrier in a training window, 14 .. 17 and 23 .. 26 (50 <= 67.5 - 10)
    assert np.flatnonzero(R.detect(row, 2, 4, -10, R.GO)[0]).tolist() == list(range(0, 14)) + [18, 19, 20, 21, 22] + list(range(27, 40))
    assert not R.detect(np.full((1, 1), 200, np.uint8), 0, 1, -100, R.SO).any()     # no neighbour at all: no hit


def _bands(hits, rows, min_fraction, max_gap=0, min_width=1, capacity=None):
    got = fsea.cfar_bands(hits, rows, min_fraction, max_gap, min_width)
    want = R.bands_of(hits, rows, min_fraction, max_gap, min_width)
    assert got.dtype == fsea.CFAR_BAND == R.BAND and got.dtype.itemsize == 24
    assert np.array_equal(got, want), (hits, rows, min_fraction, max_gap, min_width, got, want)
    return [tuple(int(v) for v in b) for b in got]


def test_bands_against_the_restatement_on_random_hits():
    rng = np.random.default_rng(1)
    for _ in range(400):
        width = int(rng.integers(1, 80))
        hits = (rng.integers(0, 50, width) * (rng.random(width) < rng.random())).astype(np.uint32)
        _bands(hits, int(rng.integers(0, 60)), float(rng.random()), int(rng.integers(0, 5)), int(rng.integers(1, 6)))
    big = np.full(9, 0xffffffff, np.uint32)
    assert _bands(big, (1 << 32) - 1, 1.0) == [(0, 8, 0, 0xffffffff, 9 * 0xffffffff)]


def test_bands_on_columns_one_can_read_off():
    z = np.zeros(12, np.uint32)
    assert _bands(z, 10, 0.5) == [] and _bands(z[:1], 10, 0.0) == []
    one = z.copy()
    one[7] = 5
    assert _bands(one, 10, 0.5) == [(7, 7, 7, 5, 5)] and _bands(one, 10, 0.51) == []           # c_min = 5, then 6
    two = np.array([0, 9, 9, 0, 0, 0, 8, 9, 0, 0, 0, 0], np.uint32)
    assert _bands(two, 10, 0.5, max_gap=3) == [(1, 7, 1, 9, 35)]                                # joined by max_gap 3 ...
    assert _bands(two, 10, 0.5, max_gap=2) == [(1, 2, 1, 9, 18), (6, 7, 7, 9, 17)]              # ... and not by 2
    assert _bands(two, 10, 0.85, max_gap=4) == [(1, 7, 1, 9, 35)]                               # c_min 9: the 8 is a fourth gap column
    assert _bands(two, 10, 0.85, max_gap=3) == [(1, 2, 1, 9, 18), (7, 7, 7, 9, 9)]
    assert _bands(two, 10, 0.85, max_gap=3, min_width=2) == [(1, 2, 1, 9, 18)]                  # a run dropped by min_width
    tie = np.array([3, 7, 2, 7, 7, 1], np.uint32)
    assert _bands(tie, 7, 0.1) == [(0, 5, 1, 7, 27)]                                            # the lowest column wins
    assert _bands(tie, 0, 0.0) == [] and _bands(tie, 0, 1.0) == []                              # rows == 0: no band
    assert _bands(tie, 7, 0.0) == [(0, 5, 1, 7, 27)]                                            # c_min = max(1, 0) = 1
    assert _bands(np.array([0, 1, 0], np.uint32), 7, 0.0) == [(1, 1, 1, 1, 1)]
    assert _bands(tie, 7, 1.0) == [(1, 1, 1, 7, 7), (3, 4, 3, 7, 14)]


def test_bands_with_a_capacity_below_the_number_found():
    L = fsea.hip_lib()
    hits = np.array([5, 0, 5, 0, 5, 0, 5], np.uint32)
    out = np.zeros(3, fsea.CFAR_BAND)
    out["first"] = -7
    n = ctypes.c_size_t()
    assert L.fsea_cfar_bands(hits.ctypes.data, 7, 5, 1.0, 0, 1, out.ctypes.data, 2, ctypes.byref(n)) == 0
    assert n.value == 4 and out["first"].tolist() == [0, 2, -7]                  # two written, four found
    assert L.fsea_cfar_bands(hits.ctypes.data, 7, 5, 1.0, 0, 1, None, 0, ctypes.byref(n)) == 0 and n.value == 4


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()

    def define(name):
        return eval(re.search(r"#define %s (\(1 << \d+\)|\d+)" % name, text).group(1))

    assert define("FSEA_CFAR_MAX_WIDTH") == fsea.CFAR_MAX_WIDTH == 1 << 20
    assert define("FSEA_CFAR_MAX_GUARD") == fsea.CFAR_MAX_GUARD == R.MAX_GUARD == 64
    assert define("FSEA_CFAR_MAX_TRAIN") == fsea.CFAR_MAX_TRAIN == R.MAX_TRAIN == 256
    assert define("FSEA_CFAR_MAX_OFFSET") == fsea.CFAR_MAX_OFFSET == R.MAX_OFFSET == 1 << 20
    assert define("FSEA_CFAR_F32_SCALE") == fsea.CFAR_F32_SCALE == R.F32_SCALE == 64
    assert define("FSEA_CFAR_TILE_COLUMNS") == fsea.CFAR_TILE_COLUMNS
    assert define("FSEA_CFAR_RUN_ROWS") == fsea.CFAR_RUN_ROWS
    for names, values in (("FSEA_CFAR_U8 = 0, FSEA_CFAR_F32 = 1", (fsea.CFAR_U8, fsea.CFAR_F32)),
                          ("FSEA_CFAR_CA = 0, FSEA_CFAR_GO = 1, FSEA_CFAR_SO = 2", (fsea.CFAR_CA, fsea.CFAR_GO, fsea.CFAR_SO))):
        assert "enum { %s }" % names in text and values == tuple(range(len(values)))
    assert (R.U8, R.F32) == (0, 1) and (R.CA, R.GO, R.SO) == (0, 1, 2)


def test_cfar_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    h = ctypes.c_void_p()
    for width in (0, -1, fsea.CFAR_MAX_WIDTH + 1):
        assert L.fsea_cfar_create(ctypes.byref(h), width, 0) == FSEA_EINVAL and not h.value, width
        assert b"width" in err()
    assert L.fsea_cfar_create(None, 64, 0) == FSEA_EINVAL and b"out-pointer" in err()

    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    # a NULL object
    assert L.fsea_cfar_add_device(None, p, 0, 1, 64, None, None, None) == FSEA_EINVAL and b"cfar is NULL" in err()
    assert L.fsea_cfar_add_host(None, p, 0, 1, 64, None, None) == FSEA_EINVAL and b"cfar is NULL" in err()
    assert L.fsea_cfar_reset(None) == FSEA_EINVAL and b"cfar is NULL" in err()
    assert L.fsea_cfar_set(None, 2, 16, 60, 0) == FSEA_EINVAL and b"cfar is NULL" in err()
    assert L.fsea_cfar_hits_host(None, p) == FSEA_EINVAL and b"cfar is NULL" in err()
    assert L.fsea_cfar_destroy(None) == 0
    assert L.fsea_cfar_width(None) == 0 and L.fsea_cfar_rows(None) == 0

    # a fake object: the struct begins with `int width; int device; uint64_t rows;` and the four settings; the remaining
    # checks run before anything else of it is used
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iiQ", fake, 0, 64, 0, 0)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert L.fsea_cfar_width(f) == 64 and L.fsea_cfar_rows(f) == 0
    for add, tail in ((L.fsea_cfar_add_device, (None, None, None)), (L.fsea_cfar_add_host, (None, None))):
        for bad_type in (-1, 2, 7):
            assert add(f, p, bad_type, 1, 64, *tail) == FSEA_EINVAL and b"type" in err()
        assert add(f, p, 0, (1 << 31) + 1, 64, *tail) == FSEA_EINVAL and b"n_rows" in err()
        assert add(f, None, 0, 1, 64, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        for pitch in (0, 1, 63):
            assert add(f, p, 0, 1, pitch, *tail) == FSEA_EINVAL and b"pitch" in err()
        assert add(f, None, 0, 0, 64, *tail) == 0                                # n_rows == 0: a successful no-op
        assert add(f, p, 1, 0, 0, *tail) == 0
    for off in (1, 4, 8):
        assert L.fsea_cfar_add_device(f, p + off, 0, 1, 64, None, None, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_cfar_add_device(f, p, 0, 1, 64, p + 1024 + off, None, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_cfar_add_device(f, p, 0, 1, 64, None, p + 2048 + off, None) == FSEA_EINVAL and b"aligned" in err()
    # rows would pass 2^32 - 1
    struct.pack_into("<iiQ", fake, 0, 64, 0, (1 << 32) - 2)
    assert L.fsea_cfar_add_device(f, p, 0, 2, 64, None, None, None) == FSEA_EINVAL and b"2^32 - 1" in err()
    assert L.fsea_cfar_add_host(f, p, 0, 2, 64, None, None) == FSEA_EINVAL and b"2^32 - 1" in err()
    struct.pack_into("<iiQ", fake, 0, 64, 0, 0)
    # the settings
    for guard in (-1, fsea.CFAR_MAX_GUARD + 1):
        assert L.fsea_cfar_set(f, guard, 16, 60, 0) == FSEA_EINVAL and b"guard" in err()
    for train in (0, -1, fsea.CFAR_MAX_TRAIN + 1):
        assert L.fsea_cfar_set(f, 2, train, 60, 0) == FSEA_EINVAL and b"train" in err()
    for offset in (fsea.CFAR_MAX_OFFSET + 1, -fsea.CFAR_MAX_OFFSET - 1):
        assert L.fsea_cfar_set(f, 2, 16, offset, 0) == FSEA_EINVAL and b"offset" in err()
    for method in (-1, 3):
        assert L.fsea_cfar_set(f, 2, 16, 60, method) == FSEA_EINVAL and b"method" in err()
    assert L.fsea_cfar_set(f, fsea.CFAR_MAX_GUARD, fsea.CFAR_MAX_TRAIN, -fsea.CFAR_MAX_OFFSET, 2) == 0
    assert struct.unpack_from("<iiii", fake, 16) == (64, 256, -(1 << 20), 2)
    assert L.fsea_cfar_hits_host(f, None) == FSEA_EINVAL and b"hits is NULL" in err()

    # the bands: host arithmetic
    hits = np.zeros(8, np.uint32)
    out = np.zeros(8, fsea.CFAR_BAND)
    n = ctypes.c_size_t()
    hp, op, np_ = hits.ctypes.data, out.ctypes.data, ctypes.byref(n)
    assert L.fsea_cfar_bands(None, 8, 1, 0.5, 0, 1, op, 8, np_) == FSEA_EINVAL and b"NULL" in err()
    assert L.fsea_cfar_bands(hp, 8, 1, 0.5, 0, 1, op, 8, None) == FSEA_EINVAL and b"NULL" in err()
    assert L.fsea_cfar_bands(hp, 8, 1, 0.5, 0, 1, None, 8, np_) == FSEA_EINVAL and b"NULL" in err()
    for width in (0, -3, fsea.CFAR_MAX_WIDTH + 1):
        assert L.fsea_cfar_bands(hp, width, 1, 0.5, 0, 1, op, 8, np_) == FSEA_EINVAL and b"width" in err()
    for fraction in (-0.01, 1.01, float("nan"), float("inf")):
        assert L.fsea_cfar_bands(hp, 8, 1, fraction, 0, 1, op, 8, np_) == FSEA_EINVAL and b"min_fraction" in err()
    assert L.fsea_cfar_bands(hp, 8, 1, 0.5, -1, 1, op, 8, np_) == FSEA_EINVAL and b"max_gap" in err()
    for min_width in (0, -1):
        assert L.fsea_cfar_bands(hp, 8, 1, 0.5, 0, min_width, op, 8, np_) == FSEA_EINVAL and b"min_width" in err()
    assert L.fsea_cfar_bands(hp, 8, 1, 1.0, 0, 1, op, 8, np_) == 0 and n.value == 0


def test_no_gpu_create_says_so():
    if fsea.device_count() > 0:
        pytest.skip("a GPU is present")
    h = ctypes.c_void_p()
    assert fsea.hip_lib().fsea_cfar_create(ctypes.byref(h), 64, 0) == -2 and not h.value       # FSEA_ENODEVICE


def _child(body, env=""):
    code = ("import os, sys; sys.path.insert(0, %r)\n%s"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n%s\nprint('returned')\n") % (ROOT, env, body)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("body,text", [
    ("L.nrf_spectrum_occupancy_new(0, 64, 2, 16, 60, 0)", "fft size 0"),
    ("L.nrf_spectrum_occupancy_new(%d, 64, 2, 16, 60, 0)" % (fsea.CFAR_MAX_WIDTH + 1), "fft size %d" % (fsea.CFAR_MAX_WIDTH + 1)),
    ("L.nrf_spectrum_occupancy_new(128, 0, 2, 16, 60, 0)", "hop 0"),
    ("L.nrf_spectrum_occupancy_new(128, 128, -1, 16, 60, 0)", "guard -1"),
    ("L.nrf_spectrum_occupancy_new(128, 128, 65, 16, 60, 0)", "guard 65"),
    ("L.nrf_spectrum_occupancy_new(128, 128, 2, 0, 60, 0)", "train 0"),
    ("L.nrf_spectrum_occupancy_new(128, 128, 2, 257, 60, 0)", "train 257"),
    ("L.nrf_spectrum_occupancy_new(128, 128, 2, 16, 1048577, 0)", "offset 1048577"),
    ("L.nrf_spectrum_occupancy_new(128, 128, 2, 16, 60, 3)", "method 3"),
])
def test_occupancy_block_with_bad_arguments_exits(body, text):
    r = _child(body)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF SPECTRUM OCCUPANCY fatal error: " + text in r.stderr


def test_occupancy_block_backend_failure_exits():
    """A device that does not exist, with or without a GPU in the machine: the backend's status and text, then exit."""
    r = _child("L.nrf_spectrum_occupancy_new(128, 128, 2, 16, 60, 0)", env="os.environ['NRF_FFT_DEVICE'] = '4096'\n")
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF SPECTRUM OCCUPANCY fatal error: fsea_plan_create failed" in r.stderr


def test_occupancy_is_an_addition_in_the_full_host_library_only():
    names = [n for n in nrf.NRF_ADDITIONS if n.startswith("nrf_spectrum_occupancy_")]
    assert len(names) == 6 and not set(names) & set(nrf.NRF_EXPORTS)
    pkg = os.path.join(ROOT, "frequensea_amd")
    full = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pkg, "libfsea_nrf.so")], capture_output=True,
                          text=True, check=True).stdout.split()
    assert set(names) <= set(full)
    fft_only = os.path.join(pkg, "libfsea_nrf_fft.so")
    if os.path.exists(fft_only):
        syms = subprocess.run(["nm", "-D", "--defined-only", fft_only], capture_output=True, text=True, check=True).stdout
        assert "nrf_spectrum_occupancy" not in syms
    assert len([n for n in fsea.EXPORTS if n.startswith("fsea_cfar_")]) == 10


def test_tool_usage_message(tmp_path):
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: fsea-occupancy FILE --size N")
    for flag in ("--hop", "--window", "--flip", "--mode db5|db10|db", "--guard", "--train", "--offset LEVELS", "--method ca|go|so",
                 "--min-duty", "--max-gap", "--min-width", "--rate HZ --freq MHZ", "--mask OUT.png", "--bands FILE", "--image IN.png"):
        assert flag in r.stdout, flag
    x = ["x.raw", "--size", "64"]
    for args, text in (([], "no recording file given"), (["x.raw"], "--size"), (["x.raw", "--size", "0"], "--size"),
                       (x + ["--hop", "-1"], "--hop"), (x + ["--method", "os"], "--method"), (x + ["--mode", "db7"], "--mode"),
                       (x + ["--guard", "65"], "--guard"), (x + ["--train", "0"], "--train"), (x + ["--offset", "2000000"], "--offset"),
                       (x + ["--min-duty", "1.5"], "--min-duty"), (x + ["--max-gap", "-1"], "--max-gap"),
                       (x + ["--min-width", "0"], "--min-width"), (x + ["--rate", "8e6"], "go together"),
                       (x + ["--image", "y.png"], "not both"), (x + ["--bogus"], "usage: fsea-occupancy"),
                       (["--image", str(tmp_path / "missing.png")], "cannot read"),
                       ([str(tmp_path / "missing.raw"), "--size", "64"], "cannot open recording")):
        r = subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)


def test_shipped_library_has_the_cfar_kernels_within_their_budget():
    """The add kernels (16-byte and element-wise forms): wave64, 256 lanes, no scratch, at most 128 VGPRs and at most 80 KiB
    of static LDS, so that two workgroups fit a CU's 160 KiB: four waves' prefix arrays (336 zero dwords in front of
    1024 + 2 * 320 + 16 cells) and level arrays (1024) and the run's 1024 column totals, 52 736 bytes."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    lds = (4 * (336 + 1024 + 2 * (fsea.CFAR_MAX_GUARD + fsea.CFAR_MAX_TRAIN) + 16 + 1024) + 1024) * 4
    assert fsea.CFAR_TILE_COLUMNS == 1024 and lds == 52736
    for name in ("fsea_cfar_u8", "fsea_cfar_f32", "fsea_cfar_u8_narrow", "fsea_cfar_f32_narrow"):
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".sgpr_spill_count"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] == lds <= 80 * 1024, (name, k[".group_segment_fixed_size"])
    assert fsea.CFAR_RUN_ROWS % 4 == 0 and fsea.CFAR_RUN_ROWS // 4 <= 255       # a lane counts a column's hits in a byte
