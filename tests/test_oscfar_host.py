"""CPU tier: the ordered-statistic CFAR detector without a GPU -- the two numpy restatements of tests/oscfar_ref.py against
each other, the cases one can read off, the argument checks of fsea_oscfar_* (before any device work), the header's
constants, the tools' --rank option and the shipped kernels' resource usage.  Every comparison is exact."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import cfar_ref as C
from tests import oscfar_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
BIN = os.path.join(ROOT, "frequensea_amd", "bin")
LIMIT = 1 << 20


def _both(rows, *settings):
    a, b = R.detect(rows, *settings), R.detect_loops(rows, *settings)
    assert np.array_equal(a, b), (rows.shape, settings, np.argwhere(a != b)[:4].tolist())
    return a


@pytest.mark.parametrize("first", range(1, 81, 10))
def test_the_two_restatements_agree(first):
    """Widths 1 .. 80, ten to a case; random G, T and R, offsets of both signs; full-range rows, rows of few distinct levels
    (ties decide) and f32 rows with NaN, +-inf and values at and beyond the clamps."""
    for width in range(first, first + 10):
        rng = np.random.default_rng(width)
        for _ in range(4):
            G, T = int(rng.integers(0, 5)), int(rng.integers(1, 41))
            rank = int(rng.integers(1, 2 * T + 1))
            offset = int(rng.integers(-30, 31))
            rows = rng.integers(0, 256, (3, width), dtype=np.uint8)
            rows[1] = rng.integers(100, 104, width)                                 # four levels: many ties
            rows[2] = 7 * rng.integers(0, 2, width)
            _both(rows, G, T, offset, rank)
            _both(rows, G, T, 0, rank)
            f = rng.normal(-60, 8, (2, width)).astype(np.float32)
            special = np.array([np.nan, np.inf, -np.inf, 16384.0, -16384.0, 16383.99, -16383.99, 1e30, -1e30, 0.5 / 64], np.float32)
            where = rng.random(f.shape) < 0.3
            f[where] = special[rng.integers(0, special.size, int(where.sum()))]
            for off in (offset * 64, -LIMIT, LIMIT, 0):
                _both(f, G, T, off, rank)


def test_the_worked_case():
    """A u8 row of 128 cells at level 100, a carrier of 200 on columns 40 .. 47 and one of 130 on column 60, G = 2, T = 16,
    offset 20: CA hits 40 .. 47 only (column 60 sees a window mean of 118.75), rank 24 of 32 hits 40 .. 47 and 60."""
    row = np.full((1, 128), 100, np.uint8)
    row[0, 40:48] = 200
    row[0, 60] = 130
    assert np.flatnonzero(_both(row, 2, 16, 20, 24)[0]).tolist() == list(range(40, 48)) + [60]
    assert np.flatnonzero(C.detect(row, 2, 16, 20, C.CA)[0]).tolist() == list(range(40, 48))
    window = [int(v) for v in row[0, 42:58]] + [int(v) for v in row[0, 63:79]]
    assert sum(window) / 32 == 118.75 and sorted(window)[23] == 100


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 19, 40])
def test_constant_rows_and_rows_narrower_than_the_guard(width):
    """A constant row: no hit at offset >= 0 (x > z + offset is strict), and at offset -1 a hit in every cell that has a
    training cell inside the row.  A row narrower than G + 2 has none anywhere."""
    G, T = 2, 16
    rows = np.full((2, width), 77, np.uint8)
    for offset in (0, 1, 60):
        assert not _both(rows, G, T, offset, 24).any()
    loL, hiL, loR, hiR = R.windows(width, G, T)
    n = (hiL - loL) + (hiR - loR)
    got = _both(rows, G, T, -1, 24)
    assert np.array_equal(got[0] == 255, n > 0) and np.array_equal(got[0], got[1])
    assert (width < G + 2) == (not n.any())
    if width < G + 2:
        assert not _both(np.random.default_rng(width).integers(0, 256, (3, width), dtype=np.uint8), G, T, -LIMIT, 1).any()


def test_rank_1_and_rank_2t_are_the_minimum_and_the_maximum():
    rng = np.random.default_rng(2)
    G, T, width = 1, 5, 60
    rows = rng.integers(0, 50, (4, width), dtype=np.uint8)
    x = rows.astype(np.int64)
    for rank, pick in ((1, min), (2 * T, max)):
        want = np.zeros(rows.shape, np.uint8)
        for r in range(4):
            for k in range(width):
                cells = [x[r, c] for c in list(range(k - G - T, k - G)) + list(range(k + G + 1, k + G + T + 1)) if 0 <= c < width]
                want[r, k] = 255 if x[r, k] > pick(cells) + 3 else 0
        assert np.array_equal(_both(rows, G, T, 3, rank), want), rank
    # r = ceil(R n / 2T): R for a whole window, at least 1 and at most n for a clipped one
    for T in (1, 3, 16, 256):
        for rank in (1, T, 2 * T):
            n = np.arange(1, 2 * T + 1)
            r = R.rank_of(n, T, rank)
            assert r[-1] == rank and (r >= 1).all() and (r <= n).all() and np.array_equal(r, np.ceil(rank * n / (2 * T)).astype(int))


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()

    def define(name):
        return eval(re.search(r"#define %s (\(1 << \d+\)|\d+)" % name, text).group(1))

    assert define("FSEA_OSCFAR_TILE_COLUMNS") == fsea.OSCFAR_TILE_COLUMNS
    assert define("FSEA_OSCFAR_RUN_ROWS") == fsea.OSCFAR_RUN_ROWS
    names = sorted(n for n in fsea.EXPORTS if n.startswith("fsea_oscfar_"))
    assert names == sorted("fsea_oscfar_" + n for n in ("create", "destroy", "reset", "set", "width", "rows", "rank", "add_device",
                                                        "add_host", "hits_host"))
    assert R.DEFAULT == (2, 16, 60, 24)
    assert len([n for n in fsea.EXPORTS if n.startswith("fsea_cfar_")]) == 10          # nothing was added under that prefix


def test_oscfar_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    h = ctypes.c_void_p()
    for width in (0, -1, fsea.CFAR_MAX_WIDTH + 1):
        assert L.fsea_oscfar_create(ctypes.byref(h), width, 0) == FSEA_EINVAL and not h.value, width
        assert b"width" in err()
    assert L.fsea_oscfar_create(None, 64, 0) == FSEA_EINVAL and b"out-pointer" in err()

    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    # a NULL object
    assert L.fsea_oscfar_add_device(None, p, 0, 1, 64, None, None, None) == FSEA_EINVAL and b"oscfar is NULL" in err()
    assert L.fsea_oscfar_add_host(None, p, 0, 1, 64, None, None) == FSEA_EINVAL and b"oscfar is NULL" in err()
    assert L.fsea_oscfar_reset(None) == FSEA_EINVAL and b"oscfar is NULL" in err()
    assert L.fsea_oscfar_set(None, 2, 16, 60, 24) == FSEA_EINVAL and b"oscfar is NULL" in err()
    assert L.fsea_oscfar_hits_host(None, p) == FSEA_EINVAL and b"oscfar is NULL" in err()
    assert L.fsea_oscfar_destroy(None) == 0
    assert L.fsea_oscfar_width(None) == 0 and L.fsea_oscfar_rows(None) == 0 and L.fsea_oscfar_rank(None) == 0

    # a fake object: the struct begins with `int width; int device; uint64_t rows;` and the four settings; the remaining
    # checks run before anything else of it is used
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iiQiiii", fake, 0, 64, 0, 0, 2, 16, 60, 24)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert L.fsea_oscfar_width(f) == 64 and L.fsea_oscfar_rows(f) == 0 and L.fsea_oscfar_rank(f) == 24
    for add, tail in ((L.fsea_oscfar_add_device, (None, None, None)), (L.fsea_oscfar_add_host, (None, None))):
        for bad_type in (-1, 2, 7):
            assert add(f, p, bad_type, 1, 64, *tail) == FSEA_EINVAL and b"type" in err()
        assert add(f, p, 0, (1 << 31) + 1, 64, *tail) == FSEA_EINVAL and b"n_rows" in err()
        assert add(f, None, 0, 1, 64, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        for pitch in (0, 1, 63):
            assert add(f, p, 0, 1, pitch, *tail) == FSEA_EINVAL and b"pitch" in err()
        assert add(f, p, 0, 1 << 31, 1 << 10, *tail) == FSEA_EINVAL and b"too large" in err()
        assert add(f, None, 0, 0, 64, *tail) == 0                                # n_rows == 0: a successful no-op
        assert add(f, p, 1, 0, 0, *tail) == 0
        # fsea_cfar's order: the type before n_rows, n_rows before the buffer, the buffer before the pitch
        assert add(f, None, 9, (1 << 31) + 1, 0, *tail) == FSEA_EINVAL and b"type" in err()
        assert add(f, None, 0, (1 << 31) + 1, 0, *tail) == FSEA_EINVAL and b"n_rows" in err()
        assert add(f, None, 0, 1, 0, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
    for off in (1, 4, 8):
        assert L.fsea_oscfar_add_device(f, p + off, 0, 1, 64, None, None, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_oscfar_add_device(f, p, 0, 1, 64, p + 1024 + off, None, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_oscfar_add_device(f, p, 0, 1, 64, None, p + 2048 + off, None) == FSEA_EINVAL and b"aligned" in err()
    # rows would pass 2^32 - 1
    struct.pack_into("<iiQ", fake, 0, 64, 0, (1 << 32) - 2)
    assert L.fsea_oscfar_add_device(f, p, 0, 2, 64, None, None, None) == FSEA_EINVAL and b"2^32 - 1" in err()
    assert L.fsea_oscfar_add_host(f, p, 0, 2, 64, None, None) == FSEA_EINVAL and b"2^32 - 1" in err()
    struct.pack_into("<iiQ", fake, 0, 64, 0, 0)
    # the settings, each refusal with its word
    for guard in (-1, fsea.CFAR_MAX_GUARD + 1):
        assert L.fsea_oscfar_set(f, guard, 16, 60, 24) == FSEA_EINVAL and b"guard" in err()
    for train in (0, -1, fsea.CFAR_MAX_TRAIN + 1):
        assert L.fsea_oscfar_set(f, 2, train, 60, 24) == FSEA_EINVAL and b"train" in err()
    for offset in (fsea.CFAR_MAX_OFFSET + 1, -fsea.CFAR_MAX_OFFSET - 1):
        assert L.fsea_oscfar_set(f, 2, 16, offset, 24) == FSEA_EINVAL and b"offset" in err()
    for train, rank in ((16, 0), (16, -1), (16, 33), (1, 3), (256, 513)):
        assert L.fsea_oscfar_set(f, 2, train, 60, rank) == FSEA_EINVAL and b"rank" in err()
    # ... in the order guard, train, offset, rank: the first bad one is named
    assert L.fsea_oscfar_set(f, -1, 0, 1 << 21, 0) == FSEA_EINVAL and b"guard" in err()
    assert L.fsea_oscfar_set(f, 0, 0, 1 << 21, 0) == FSEA_EINVAL and b"train" in err()
    assert L.fsea_oscfar_set(f, 0, 1, 1 << 21, 0) == FSEA_EINVAL and b"offset" in err()
    assert L.fsea_oscfar_set(f, 0, 1, 0, 0) == FSEA_EINVAL and b"rank" in err()
    assert struct.unpack_from("<iiii", fake, 16) == (2, 16, 60, 24)              # a refused call changes nothing
    assert L.fsea_oscfar_set(f, fsea.CFAR_MAX_GUARD, fsea.CFAR_MAX_TRAIN, -fsea.CFAR_MAX_OFFSET, 512) == 0
    assert struct.unpack_from("<iiii", fake, 16) == (64, 256, -(1 << 20), 512) and L.fsea_oscfar_rank(f) == 512
    assert L.fsea_oscfar_set(f, 0, 1, fsea.CFAR_MAX_OFFSET, 1) == 0 and L.fsea_oscfar_set(f, 0, 1, 0, 2) == 0
    assert L.fsea_oscfar_hits_host(f, None) == FSEA_EINVAL and b"hits is NULL" in err()


def test_no_gpu_create_says_so():
    if fsea.device_count() > 0:
        pytest.skip("a GPU is present")
    h = ctypes.c_void_p()
    assert fsea.hip_lib().fsea_oscfar_create(ctypes.byref(h), 64, 0) == -2 and not h.value       # FSEA_ENODEVICE


@pytest.mark.parametrize("tool,head", [("fsea-occupancy", ["x.raw", "--size", "64"]), ("fsea-events", ["x.raw", "--size", "64"]),
                                       ("fsea-cutouts", ["x.raw", "--size", "64", "--decimation", "4", "--out", "d"])])
def test_tools_usage_and_usage_errors_of_rank(tool, head):
    path = os.path.join(BIN, tool)
    r = subprocess.run([path, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: %s FILE --size N" % tool)
    assert "--rank R" in r.stdout and "--method ca|go|so" in r.stdout
    for args, text in ((["--rank", "0"], "--rank must be in"), (["--rank", "-3"], "--rank must be in"), (["--rank", "33"], "--rank must be in"),
                       (["--train", "4", "--rank", "9"], "--rank must be in"), (["--rank", "24", "--method", "ca"], "--method"),
                       (["--method", "so", "--rank", "24"], "--rank"), (["--method", "os"], "--method must be ca, go or so"),
                       (["--rank"], "usage: " + tool)):
        r = subprocess.run([path] + head + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr and not r.stdout, (args, r.stderr)
    # a rank that fits the train asked for passes the option checks: the next complaint is the missing recording's
    r = subprocess.run([path] + head + ["--train", "40", "--rank", "80"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--rank" not in r.stderr and "cannot open recording" in r.stderr, r.stderr


def test_shipped_library_has_the_oscfar_kernels_within_their_budget():
    """The add kernels (16-byte and element-wise forms): wave64, 256 lanes, no scratch, no spilled vector register, at most
    128 VGPRs and at most 80 KiB of static LDS, so that two workgroups fit a CU's 160 KiB.  Four waves' level arrays (1024
    cells and a halo of 320 each side, int32) and the run's 1024 column totals: 30 720 bytes.  As built: 75 VGPRs for
    fsea_oscfar_u8, 104 for fsea_oscfar_f32, 63 and 75 for their _narrow forms; the compiler parks 30, 76, 14 and 20 scalar
    values in lanes of a vector register (no memory traffic)."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    lds = (4 * (1024 + 2 * 320) + 1024) * 4
    assert fsea.OSCFAR_TILE_COLUMNS == 1024 and fsea.CFAR_MAX_GUARD + fsea.CFAR_MAX_TRAIN == 320 and lds == 30720
    for name in ("fsea_oscfar_u8", "fsea_oscfar_f32", "fsea_oscfar_u8_narrow", "fsea_oscfar_f32_narrow"):
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".sgpr_spill_count"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] == lds <= 80 * 1024, (name, k[".group_segment_fixed_size"])
    assert fsea.OSCFAR_RUN_ROWS % 4 == 0 and fsea.OSCFAR_RUN_ROWS // 4 <= 255   # a lane counts a column's hits in a byte
