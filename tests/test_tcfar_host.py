"""CPU tier: the time-axis CFAR detector without a GPU -- the two numpy restatements of tests/tcfar_ref.py against each
other, the worked case of include/fsea.h, the argument checks of fsea_tcfar_* (before any device work) with their texts, the
header's constants, the tools' --axis usage errors and the shipped kernels' resource usage."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import cfar_ref as R
from tests import tcfar_ref as TR
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
TCFAR = fsea.Tcfar      # the restatements are of this object: without it no test of this file says anything
BIN = os.path.join(ROOT, "frequensea_amd", "bin")
SPECIAL_F32 = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 16384.0, -16384.0, 16383.99, -16383.99, 0.0, -0.0, 3e38, -3e38,
                        0.5 / 64, 1.5 / 64, 2.5 / 64, -0.5 / 64, -1.5 / 64, 20000.0, -20000.0], np.float32)


def _random_call(rng, rows_max=40, cols_max=9):
    total, width = int(rng.integers(1, rows_max + 1)), int(rng.integers(1, cols_max + 1))
    before = int(rng.integers(0, total))
    n = int(rng.integers(1, total - before + 1))
    return total, width, before, n


@pytest.mark.parametrize("seed", range(6))
def test_the_two_restatements_agree(seed):
    """Blocks of 1 .. 40 rows x 1 .. 9 columns, random G, T, method and context, offsets of both signs, u8 rows with few
    distinct levels; f32 rows with NaN, +-inf, values at and beyond the clamps and half-way ties; offsets +-2^20 and 0."""
    rng = np.random.default_rng(seed)
    for _ in range(60):
        total, width, before, n = _random_call(rng)
        G, T, method = int(rng.integers(0, 5)), int(rng.integers(1, 21)), int(rng.integers(0, 3))
        offset = int(rng.choice([-7, -1, 0, 1, 5, 20]))
        block = rng.integers(100, 104, (total, width), dtype=np.uint8)       # few distinct levels: many near-ties
        if rng.random() < 0.5:
            block[rng.integers(0, total)] += 60
        a, b = TR.detect(block, before, n, G, T, offset, method), TR.detect_loops(block, before, n, G, T, offset, method)
        assert a.shape == (n, width) and np.array_equal(a, b), (total, width, before, n, G, T, offset, method)
    for _ in range(40):
        total, width, before, n = _random_call(rng)
        G, T, method = int(rng.integers(0, 4)), int(rng.integers(1, 12)), int(rng.integers(0, 3))
        block = rng.uniform(-120, 20, (total, width)).astype(np.float32)
        where = rng.random(block.shape) < 0.4
        block[where] = SPECIAL_F32[rng.integers(0, SPECIAL_F32.size, int(where.sum()))]
        for offset in (-(1 << 20), 0, 1 << 20, 3 * 64, -64):
            a, b = TR.detect(block, before, n, G, T, offset, method), TR.detect_loops(block, before, n, G, T, offset, method)
            assert np.array_equal(a, b), (total, width, before, n, G, T, offset, method)


def worked_case():
    rows = np.full((64, 256), 100, np.uint8)
    rows[30:36, 40:200] = 160
    rows[:, 220] = 200
    return rows


def test_the_worked_case_of_the_header():
    """64 rows of 256 cells at 100, a burst of 160 on rows 30 .. 35 and columns 40 .. 199, a carrier of 200 on column 220;
    (2, 16, 20, CA).  Per row: the burst's two edges only and the carrier in all 64 rows; per column: all 960 cells of the
    burst and no cell of the carrier."""
    rows = worked_case()
    freq = R.detect(rows, 2, 16, 20, R.CA)
    burst = np.zeros(rows.shape, bool)
    burst[30:36, 40:200] = True
    assert sorted(set(np.nonzero(freq[burst.any(axis=1)][:, :210])[1].tolist())) == list(range(40, 48)) + list(range(192, 200))
    assert (freq[30:36, 40:48] == 255).all() and (freq[30:36, 192:200] == 255).all() and not freq[30:36, 48:192].any()
    assert (freq[:, 220] == 255).all() and int((freq == 255).sum()) == 6 * 16 + 64
    time = TR.detect(rows, 0, 64, 2, 16, 20, TR.CA)
    assert (time[burst] == 255).all() and int((time == 255).sum()) == 960 and not time[:, 220].any()
    assert np.array_equal(TR.combine(freq, time, TR.MASK_OR) == 255, (freq == 255) | burst)
    assert int((TR.combine(freq, time, TR.MASK_AND) == 255).sum()) == 6 * 16


def test_constant_blocks_and_short_blocks():
    for total in (1, 2, 5, 19, 40):
        block = np.full((total, 3), 77, np.uint8)
        for G, T in ((0, 1), (2, 16), (3, 4)):
            for method in (TR.CA, TR.GO, TR.SO):
                assert not TR.detect(block, 0, total, G, T, 0, method).any()          # x * n > S is strict
                assert not TR.detect(block, 0, total, G, T, 5, method).any()
                got = TR.detect(block, 0, total, G, T, -1, method)
                r = np.arange(total)
                trained = (r - G - 1 >= 0) | (r + G + 1 <= total - 1)                 # some training row exists
                assert np.array_equal(got[:, 0] == 255, trained) and (got == got[:, :1]).all(), (total, G, T, method)
    rng = np.random.default_rng(1)
    for G in (0, 1, 5, 64):
        for total in range(1, G + 2):                                                 # fewer than G + 2 rows: no training row
            block = rng.integers(0, 256, (total, 4), dtype=np.uint8)
            for method in (TR.CA, TR.GO, TR.SO):
                assert not TR.detect(block, 0, total, G, 7, -1000, method).any()


def test_combine():
    old = np.array([[0, 1, 7, 255], [0, 1, 7, 255]], np.uint8)
    hit = np.array([[0, 0, 0, 0], [255, 255, 255, 255]], np.uint8)
    assert TR.combine(old, hit, TR.MASK_SET).tolist() == [[0, 0, 0, 0], [255, 255, 255, 255]]
    assert TR.combine(old, hit, TR.MASK_OR).tolist() == [[0, 255, 255, 255], [255, 255, 255, 255]]
    assert TR.combine(old, hit, TR.MASK_AND).tolist() == [[0, 0, 0, 0], [0, 255, 255, 255]]


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()

    def define(name):
        return eval(re.search(r"#define %s (\(1 << \d+\)|\d+)" % name, text).group(1))

    assert define("FSEA_TCFAR_TILE_COLUMNS") == fsea.TCFAR_TILE_COLUMNS
    assert define("FSEA_TCFAR_RUN_ROWS") == fsea.TCFAR_RUN_ROWS
    assert "enum { FSEA_TCFAR_MASK_SET = 0, FSEA_TCFAR_MASK_OR = 1, FSEA_TCFAR_MASK_AND = 2 }" in text
    assert (fsea.TCFAR_MASK_SET, fsea.TCFAR_MASK_OR, fsea.TCFAR_MASK_AND) == (TR.MASK_SET, TR.MASK_OR, TR.MASK_AND) == (0, 1, 2)
    assert sorted(n for n in fsea.EXPORTS if n.startswith("fsea_tcfar_")) == [
        "fsea_tcfar_add_device", "fsea_tcfar_add_host", "fsea_tcfar_create", "fsea_tcfar_destroy", "fsea_tcfar_hits_host",
        "fsea_tcfar_reset", "fsea_tcfar_rows", "fsea_tcfar_run_rows", "fsea_tcfar_set", "fsea_tcfar_width"]
    assert TCFAR._kind == "tcfar"


def test_tcfar_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()

    def err():
        return L.fsea_last_error_string().decode()

    h = ctypes.c_void_p()
    for width in (0, -1, fsea.CFAR_MAX_WIDTH + 1):
        assert L.fsea_tcfar_create(ctypes.byref(h), width, 0) == FSEA_EINVAL and not h.value, width
        assert err() == "width must be in [1, 1048576], got %d" % width
    assert L.fsea_tcfar_create(None, 64, 0) == FSEA_EINVAL and err() == "tcfar out-pointer is NULL"

    buf = np.zeros(8192, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    m = p + 4096
    device, host = L.fsea_tcfar_add_device, L.fsea_tcfar_add_host
    # 1. a NULL object
    assert device(None, p, 0, 1, 64, 0, 0, None, None, None) == FSEA_EINVAL and err() == "tcfar is NULL"
    assert host(None, p, 0, 1, 64, 0, 0, None, None) == FSEA_EINVAL and err() == "tcfar is NULL"
    assert L.fsea_tcfar_reset(None) == FSEA_EINVAL and err() == "tcfar is NULL"
    assert L.fsea_tcfar_set(None, 2, 16, 60, 0, 0) == FSEA_EINVAL and err() == "tcfar is NULL"
    assert L.fsea_tcfar_hits_host(None, p) == FSEA_EINVAL and err() == "tcfar is NULL"
    assert L.fsea_tcfar_destroy(None) == 0
    assert L.fsea_tcfar_width(None) == 0 and L.fsea_tcfar_rows(None) == 0 and L.fsea_tcfar_run_rows(None) == 0

    # a fake object: the struct begins with `int width; int device; uint64_t rows;` and the five settings; the remaining
    # checks run before anything else of it is used
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iiQiiiii", fake, 0, 64, 0, 0, 2, 16, 60, 0, fsea.TCFAR_MASK_OR)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert L.fsea_tcfar_width(f) == 64 and L.fsea_tcfar_rows(f) == 0 and L.fsea_tcfar_run_rows(f) == fsea.TCFAR_RUN_ROWS
    for add, tail in ((device, (None,)), (host, ())):
        def call(rows, type, n, pitch, before=0, after=0, mask=m, add=add, tail=tail):
            return add(f, rows, type, n, pitch, before, after, mask, None, *tail)
        # every later fault is present as well: the earlier check answers
        for bad_type in (-1, 2, 7):                                                  # 2. the type
            assert call(None, bad_type, (1 << 31) + 1, 0) == FSEA_EINVAL and err() == "unknown row type %d" % bad_type
        assert call(None, 0, (1 << 31) + 1, 0) == FSEA_EINVAL                        # 3. n_rows
        assert err() == "n_rows %d is more than 2^31" % ((1 << 31) + 1)
        assert call(None, 0, 3, 0, 2, 1, None) == FSEA_EINVAL                        # 4. the buffer
        assert err() == "NULL buffer for the 6 rows of the call"
        for pitch in (0, 1, 63):                                                     # 5. the pitch
            assert call(p + 1, 0, 1, pitch, 1 << 50, 0, None) == FSEA_EINVAL and err() == "pitch %d is below the width 64" % pitch
        assert call(p + 1, 0, 1 << 20, 1 << 20, 1, 0, None) == FSEA_EINVAL           # 6. the span, context included
        assert err() == "pitch 1048576 x n_rows 1048577 is too large"
        assert call(p + 1, 0, 1, 64, 1 << 62, 1 << 63, None) == FSEA_EINVAL and "is too large" in err()
        assert call(p, 0, 1 << 20, 1 << 20, 0, 0, None) == FSEA_EINVAL               # exactly 2^40: accepted by 6, refused by 8
        assert "combines with a mask" in err()
        assert call(None, 0, 0, 0, 5, 5, None) == 0                                  # n_rows == 0: a successful no-op
        assert call(None, 1, 0, 64, 0, 0, None) == 0
    for off in (1, 4, 8):                                                            # 7. the alignment, device form
        assert device(f, p + off, 0, 1, 64, 0, 0, None, None, None) == FSEA_EINVAL and "16-byte aligned" in err()
        assert device(f, p, 0, 1, 64, 0, 0, m + off, None, None) == FSEA_EINVAL and "16-byte aligned" in err()
        assert device(f, p, 0, 1, 64, 0, 0, None, m + off, None) == FSEA_EINVAL and "16-byte aligned" in err()
    # 8. OR and AND need a mask; the rows stay as they were
    struct.pack_into("<Q", fake, 8, (1 << 32) - 2)
    for op in (fsea.TCFAR_MASK_OR, fsea.TCFAR_MASK_AND):
        struct.pack_into("<i", fake, 32, op)
        assert device(f, p, 0, 2, 64, 0, 0, None, None, None) == FSEA_EINVAL
        assert err() == "mask operation %d combines with a mask, and the mask is NULL" % op
        assert host(f, p, 0, 2, 64, 0, 0, None, None) == FSEA_EINVAL
        assert err() == "mask operation %d combines with a mask, and the mask is NULL" % op
        # 9. rows would pass 2^32 - 1
        assert device(f, p, 0, 2, 64, 0, 0, m, None, None) == FSEA_EINVAL
        assert err() == "n_rows 2 would take rows past 2^32 - 1 (4294967294 so far)"
        assert host(f, p, 0, 2, 64, 0, 0, m, None) == FSEA_EINVAL and "2^32 - 1" in err()
    struct.pack_into("<i", fake, 32, fsea.TCFAR_MASK_SET)
    assert device(f, p, 0, 2, 64, 0, 0, None, None, None) == FSEA_EINVAL and "2^32 - 1" in err()
    assert L.fsea_tcfar_rows(f) == (1 << 32) - 2
    struct.pack_into("<Q", fake, 8, 0)
    # the host form's room: 2 (G + T) + 1 packed rows in the staging of 64 MiB
    struct.pack_into("<iiQiiiii", fake, 0, 1 << 20, 0, 0, 64, 256, 60, 0, 0)
    wide = np.zeros(1 << 20, np.float32)
    assert host(f, wide.ctypes.data, 1, 1, 1 << 20, 0, 0, None, None) == FSEA_EINVAL
    assert err() == ("rows of 4194304 bytes: the 641 rows of one decided row and its context do not fit the staging of 67108864 "
                     "bytes; use fsea_tcfar_add_device")
    struct.pack_into("<iiQiiiii", fake, 0, 64, 0, 0, 2, 16, 60, 0, 0)

    # the settings, in their order
    def set_(*a):
        return L.fsea_tcfar_set(f, *a)

    assert set_(-1, 0, 1 << 21, 9, 9) == FSEA_EINVAL and err() == "guard must be in [0, 64], got -1"
    assert set_(65, 16, 60, 0, 0) == FSEA_EINVAL and err() == "guard must be in [0, 64], got 65"
    assert set_(2, 0, 1 << 21, 9, 9) == FSEA_EINVAL and err() == "train must be in [1, 256], got 0"
    assert set_(2, 257, 60, 0, 0) == FSEA_EINVAL and err() == "train must be in [1, 256], got 257"
    assert set_(2, 16, (1 << 20) + 1, 9, 9) == FSEA_EINVAL and err() == "offset must be in [-1048576, 1048576], got 1048577"
    assert set_(2, 16, -(1 << 20) - 1, 0, 0) == FSEA_EINVAL and "offset" in err()
    for method in (-1, 3):
        assert set_(2, 16, 60, method, 9) == FSEA_EINVAL and err() == "unknown method %d" % method
    for op in (-1, 3):
        assert set_(2, 16, 60, 0, op) == FSEA_EINVAL and err() == "unknown mask operation %d" % op
    assert struct.unpack_from("<iiiii", fake, 16) == (2, 16, 60, 0, 0)               # a refused set changes nothing
    assert set_(fsea.CFAR_MAX_GUARD, fsea.CFAR_MAX_TRAIN, -fsea.CFAR_MAX_OFFSET, 2, 2) == 0
    assert struct.unpack_from("<iiiii", fake, 16) == (64, 256, -(1 << 20), 2, 2)
    assert L.fsea_tcfar_hits_host(f, None) == FSEA_EINVAL and err() == "hits is NULL"


def test_no_gpu_create_says_so():
    if fsea.device_count() > 0:
        pytest.skip("a GPU is present")
    h = ctypes.c_void_p()
    assert fsea.hip_lib().fsea_tcfar_create(ctypes.byref(h), 64, 0) == -2 and not h.value       # FSEA_ENODEVICE


@pytest.mark.parametrize("tool", ["fsea-occupancy", "fsea-events", "fsea-cutouts"])
def test_the_tools_axis_usage_errors(tool, tmp_path):
    """--axis in the usage text; a wrong name, --rank with --axis time, and a chunk too short for the windows are usage
    errors raised before any device call (this tier has no device)."""
    exe = os.path.join(BIN, tool)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--axis freq|time|either" in r.stdout
    raw = tmp_path / "x.raw"
    np.zeros(4096, np.uint8).tofile(raw)
    x = [str(raw), "--size", "64"]
    if tool == "fsea-cutouts":
        x += ["--decimation", "4", "--out", str(tmp_path / "cut")]
    # a chunk of N = 2^20 at hop 2^20 holds 4 frames (2^22 samples); (2, 16) asks for 37
    big = [str(raw), "--size", "1048576"] + x[3:]
    for args, text in ((x + ["--axis", "both"], "--axis must be freq, time or either"),
                       (x + ["--axis", "time", "--rank", "24"], "--rank R is across frequency: not together with --axis time"),
                       (big + ["--axis", "time"], "a chunk holds 4 frames, and --guard 2 --train 16 down the time axis need 37"),
                       (big + ["--axis", "either", "--guard", "0", "--train", "2"],
                        "a chunk holds 4 frames, and --guard 0 --train 2 down the time axis need 5")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)


def test_shipped_library_has_the_tcfar_kernels_within_their_budget():
    """The add kernels (16-byte and element-wise forms): wave64, one wave to a workgroup, no scratch, no LDS, and at most
    the registers their launch bounds leave a wave: 256 with two waves to a SIMD, 512 (vector and accumulation registers
    together) for the 16-byte f32 kernel, which holds the 16-byte groups of two rows' five reads and has a SIMD to itself."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    for name in ("fsea_tcfar_u8", "fsea_tcfar_f32", "fsea_tcfar_u8_narrow", "fsea_tcfar_f32_narrow"):
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".sgpr_spill_count"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 64, name
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= (512 if name == "fsea_tcfar_f32" else 256), (name, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
    assert fsea.TCFAR_TILE_COLUMNS == 64 * 16 and fsea.TCFAR_RUN_ROWS <= 255         # a lane counts a column's hits in a byte
