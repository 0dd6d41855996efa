"""CPU tier: the persistence spectrum without a GPU -- fsea_persist_trace against the numpy restatement of
tests/persist_ref.py, the LOG map's pinned values, the argument checks of fsea_persist_* (before any device work), the
fatal-error convention of nrf_persistence_*, the tool's usage message and the shipped kernels' resource usage."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import persist_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-persistence")


def _random_counts(width, seed):
    """Sparse random counts with an empty column, a column with one count and a column with one huge count."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1000, (256, width), dtype=np.uint32) * (rng.random((256, width)) < 0.1)
    c = c.astype(np.uint32)
    c[:, 0] = 0
    if width > 2:
        c[:, 1] = 0
        c[137, 1] = 1
        c[:, 2] = 0
        c[255, 2] = 0xffffffff
        c[0, 2] = 0xffffffff
    return c


@pytest.mark.parametrize("width", [1, 50])
def test_trace_is_the_restatement(width):
    for seed in range(4):
        c = _random_counts(width, 10 * width + seed) if seed else np.zeros((256, width), np.uint32)
        if seed == 3:
            c[:] = np.random.default_rng(3).integers(0, 1 << 32, c.shape, dtype=np.uint64).astype(np.uint32)   # dense, large
        assert np.array_equal(fsea.persist_trace(c, fsea.PERSIST_TRACE_MAX), R.trace(c, R.TRACE_MAX))
        assert np.array_equal(fsea.persist_trace(c, fsea.PERSIST_TRACE_MIN), R.trace(c, R.TRACE_MIN))
        for fraction in (0.0, 0.5, 1.0, 0.999, 1e-9):
            got = fsea.persist_trace(c, fsea.PERSIST_TRACE_QUANTILE, fraction)
            assert np.array_equal(got, R.trace(c, R.TRACE_QUANTILE, fraction)), (width, seed, fraction)


def test_trace_on_columns_one_can_read_off():
    c = np.zeros((256, 4), np.uint32)
    c[10, 1] = 1                                  # one count
    c[[3, 7, 200], 2] = [1, 2, 1]                 # cumulative 1, 3, 4: the median is level 7
    c[[0, 255], 3] = [5, 5]
    assert fsea.persist_trace(c, fsea.PERSIST_TRACE_MAX).tolist() == [0, 10, 200, 255]
    assert fsea.persist_trace(c, fsea.PERSIST_TRACE_MIN).tolist() == [0, 10, 3, 0]
    assert fsea.persist_trace(c, fsea.PERSIST_TRACE_QUANTILE, 0.5).tolist() == [0, 10, 7, 0]
    assert fsea.persist_trace(c, fsea.PERSIST_TRACE_QUANTILE, 0.0).tolist() == [0, 10, 3, 0]
    assert fsea.persist_trace(c, fsea.PERSIST_TRACE_QUANTILE, 1.0).tolist() == [0, 10, 200, 255]
    assert fsea.persist_trace(c, fsea.PERSIST_TRACE_QUANTILE, 0.51).tolist() == [0, 10, 7, 255]


def test_the_log_maps_pinned_values():
    assert (R.log_q(0), R.log_q(1), R.log_q(2), R.log_q((1 << 32) - 1)) == (0, 1, 257, 8192)
    px = R.map_counts(np.array([0, 1, 2, 3, 4, 5, 999, 1000, 1001, 70000], np.uint32), R.MAP_LOG, 1000)
    assert px[:6].tolist() == [0, 1, 26, 39, 52, 58] and px[7:].tolist() == [255, 255, 255] and px[6] < 255
    every = R.map_counts(np.arange(0, 3000, dtype=np.uint32), R.MAP_LOG, 1000).astype(int)
    assert (np.diff(every) >= 0).all() and every[1] == 1                       # monotone; a single hit stays visible
    assert R.map_counts(np.array([0, 1, 5], np.uint32), R.MAP_LOG, 1).tolist() == [0, 1, 255]
    assert R.map_counts(np.array([0, 1, 5], np.uint32), R.MAP_LOG, 0).tolist() == [0, 0, 0]
    assert R.map_counts(np.array([0, 1, 254, 255, 256, 1 << 31], np.uint32), R.MAP_SATURATE, 7).tolist() == [0, 1, 254, 255, 255, 255]
    assert R.map_counts(np.array([0, 1, 127, 128, 255, 256, 300], np.uint32), R.MAP_LINEAR, 256).tolist() == [0, 0, 126, 127, 254, 255, 255]


def test_the_restatements_f32_levels_at_the_boundaries():
    """Range (-70, 30): scale 2.56.  lo, hi, just below hi, both infinities, a NaN."""
    lo, hi = np.float32(-70), np.float32(30)
    v = np.array([[lo, hi, np.nextafter(hi, np.float32(-np.inf)), -np.inf, np.inf, np.nan, -200, 200, -69.9]], np.float32)
    assert R.scale_of(lo, hi) == np.float32(2.56)
    assert R.levels_of(v, lo, hi).tolist() == [[0, 255, 255, 0, 255, -1, 0, 255, 0]]
    c = R.counts_of(v, lo, hi)
    assert c.sum() == 8 and c[:, 5].sum() == 0


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()

    def define(name):
        return int(re.search(r"#define %s (\d+)" % name, text).group(1))

    assert define("FSEA_PERSIST_LEVELS") == fsea.PERSIST_LEVELS == R.LEVELS == 256
    assert define("FSEA_PERSIST_MAX_WIDTH") == fsea.PERSIST_MAX_WIDTH == 65536
    assert define("FSEA_PERSIST_RUN_ROWS") == fsea.PERSIST_RUN_ROWS
    for names, values in (("FSEA_PERSIST_U8 = 0, FSEA_PERSIST_F32 = 1", (fsea.PERSIST_U8, fsea.PERSIST_F32)),
                          ("FSEA_PERSIST_MAP_SATURATE = 0, FSEA_PERSIST_MAP_LINEAR = 1, FSEA_PERSIST_MAP_LOG = 2",
                           (fsea.PERSIST_MAP_SATURATE, fsea.PERSIST_MAP_LINEAR, fsea.PERSIST_MAP_LOG)),
                          ("FSEA_PERSIST_TRACE_MAX = 0, FSEA_PERSIST_TRACE_MIN = 1, FSEA_PERSIST_TRACE_QUANTILE = 2",
                           (fsea.PERSIST_TRACE_MAX, fsea.PERSIST_TRACE_MIN, fsea.PERSIST_TRACE_QUANTILE))):
        assert "enum { %s }" % names in text and values == tuple(range(len(values)))
    assert (R.MAP_SATURATE, R.MAP_LINEAR, R.MAP_LOG) == (0, 1, 2) and (R.TRACE_MAX, R.TRACE_MIN, R.TRACE_QUANTILE) == (0, 1, 2)


def test_persist_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    h = ctypes.c_void_p()
    for width in (0, -1, fsea.PERSIST_MAX_WIDTH + 1):
        assert L.fsea_persist_create(ctypes.byref(h), width, 0) == FSEA_EINVAL and not h.value, width
        assert b"width" in err()
    assert L.fsea_persist_create(None, 64, 0) == FSEA_EINVAL and b"out-pointer" in err()

    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    # a NULL object
    assert L.fsea_persist_add_device(None, p, 0, 1, 64, None) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_add_host(None, p, 0, 1, 64) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_reset(None) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_set_range(None, -1.0, 1.0) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_decay(None, 1, 2, None) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_counts_host(None, p) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_image_device(None, 0, 0, p, None) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_image_host(None, 0, 0, p) == FSEA_EINVAL and b"persist is NULL" in err()
    assert L.fsea_persist_destroy(None) == 0
    assert L.fsea_persist_width(None) == 0 and L.fsea_persist_rows(None) == 0

    # a fake object: the struct begins with `int width; int device; uint64_t rows;`, the remaining checks run before
    # anything else of it is used
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iiQ", fake, 0, 64, 0, 0)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert L.fsea_persist_width(f) == 64 and L.fsea_persist_rows(f) == 0
    for add, tail in ((L.fsea_persist_add_device, (None,)), (L.fsea_persist_add_host, ())):
        for bad_type in (-1, 2, 7):
            assert add(f, p, bad_type, 1, 64, *tail) == FSEA_EINVAL and b"type" in err()
        assert add(f, p, 0, (1 << 31) + 1, 64, *tail) == FSEA_EINVAL and b"n_rows" in err()
        assert add(f, None, 0, 1, 64, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        for pitch in (0, 1, 63):
            assert add(f, p, 0, 1, pitch, *tail) == FSEA_EINVAL and b"pitch" in err()
        assert add(f, None, 0, 0, 64, *tail) == 0                                # n_rows == 0: a successful no-op
        assert add(f, p, 1, 0, 0, *tail) == 0
    for off in (1, 4, 8):
        assert L.fsea_persist_add_device(f, p + off, 0, 1, 64, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_persist_image_device(f, 0, 0, p + off, None) == FSEA_EINVAL and b"aligned" in err()
    # rows would pass 2^32 - 1
    struct.pack_into("<iiQ", fake, 0, 64, 0, (1 << 32) - 2)
    assert L.fsea_persist_add_device(f, p, 0, 2, 64, None) == FSEA_EINVAL and b"2^32 - 1" in err()
    assert L.fsea_persist_add_host(f, p, 0, 2, 64) == FSEA_EINVAL and b"2^32 - 1" in err()
    struct.pack_into("<iiQ", fake, 0, 64, 0, 0)
    # the range
    for lo, hi in ((0.0, 0.0), (1.0, -1.0), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (0.0, float("nan"))):
        assert L.fsea_persist_set_range(f, lo, hi) == FSEA_EINVAL and b"range" in err(), (lo, hi)
    assert L.fsea_persist_set_range(f, 0.0, 1e-45) == FSEA_EINVAL and b"range" in err()     # no finite f32 scale
    # the decay ratio
    for num, den in ((1, 0), (0, 0), (3, 2), (0xffffffff, 1)):
        assert L.fsea_persist_decay(f, num, den, None) == FSEA_EINVAL and b"denominator" in err(), (num, den)
    # map and buffers of the image and the counts
    for bad_map in (-1, 3):
        assert L.fsea_persist_image_host(f, bad_map, 0, p) == FSEA_EINVAL and b"map" in err()
        assert L.fsea_persist_image_device(f, bad_map, 0, p, None) == FSEA_EINVAL and b"map" in err()
    assert L.fsea_persist_image_host(f, 0, 0, None) == FSEA_EINVAL and b"image is NULL" in err()
    assert L.fsea_persist_image_device(f, 0, 0, None, None) == FSEA_EINVAL and b"image is NULL" in err()
    assert L.fsea_persist_counts_host(f, None) == FSEA_EINVAL and b"counts is NULL" in err()

    # the trace: host arithmetic
    c = np.zeros((256, 8), np.uint32)
    out = np.zeros(8, np.uint8)
    cp, op = c.ctypes.data, out.ctypes.data
    assert L.fsea_persist_trace(None, 8, 0, 0.5, op) == FSEA_EINVAL and b"NULL" in err()
    assert L.fsea_persist_trace(cp, 8, 0, 0.5, None) == FSEA_EINVAL and b"NULL" in err()
    for width in (0, -3, fsea.PERSIST_MAX_WIDTH + 1):
        assert L.fsea_persist_trace(cp, width, 0, 0.5, op) == FSEA_EINVAL and b"width" in err()
    for kind in (-1, 3):
        assert L.fsea_persist_trace(cp, 8, kind, 0.5, op) == FSEA_EINVAL and b"kind" in err()
    for fraction in (-0.01, 1.01, float("nan"), float("inf")):
        assert L.fsea_persist_trace(cp, 8, 2, fraction, op) == FSEA_EINVAL and b"fraction" in err()
    assert L.fsea_persist_trace(cp, 8, 2, 1.0, op) == 0


def test_no_gpu_create_says_so():
    if fsea.device_count() > 0:
        pytest.skip("a GPU is present")
    h = ctypes.c_void_p()
    assert fsea.hip_lib().fsea_persist_create(ctypes.byref(h), 64, 0) == -2 and not h.value       # FSEA_ENODEVICE


def _child(body, env=""):
    code = ("import os, sys; sys.path.insert(0, %r)\n%s"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n%s\nprint('returned')\n") % (ROOT, env, body)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("body,text", [
    ("L.nrf_persistence_new(0, 64, 2)", "fft size 0"),
    ("L.nrf_persistence_new(-8, 64, 2)", "fft size -8"),
    ("L.nrf_persistence_new(%d, 64, 2)" % (fsea.PERSIST_MAX_WIDTH + 1), "fft size %d" % (fsea.PERSIST_MAX_WIDTH + 1)),
    ("L.nrf_persistence_new(128, 0, 2)", "hop 0"),
    ("L.nrf_persistence_new(128, -128, 2)", "hop -128"),
    ("L.nrf_persistence_new(128, 128, 3)", "map 3"),
    ("L.nrf_persistence_new(128, 128, -1)", "map -1"),
])
def test_persistence_block_with_bad_arguments_exits(body, text):
    r = _child(body)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PERSISTENCE fatal error: " + text in r.stderr


def test_persistence_block_backend_failure_exits():
    """A device that does not exist, with or without a GPU in the machine: the backend's status and text, then exit."""
    r = _child("L.nrf_persistence_new(128, 128, 2)", env="os.environ['NRF_FFT_DEVICE'] = '4096'\n")
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PERSISTENCE fatal error: fsea_plan_create failed" in r.stderr


def test_persistence_is_an_addition_in_the_full_host_library_only():
    names = [n for n in nrf.NRF_ADDITIONS if n.startswith("nrf_persistence_")]
    assert len(names) == 6 and not set(names) & set(nrf.NRF_EXPORTS)
    pkg = os.path.join(ROOT, "frequensea_amd")
    full = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pkg, "libfsea_nrf.so")], capture_output=True,
                          text=True, check=True).stdout.split()
    assert set(names) <= set(full)
    fft_only = os.path.join(pkg, "libfsea_nrf_fft.so")
    if os.path.exists(fft_only):
        syms = subprocess.run(["nm", "-D", "--defined-only", fft_only], capture_output=True, text=True, check=True).stdout
        assert "nrf_persistence" not in syms
    assert len([n for n in fsea.EXPORTS if n.startswith("fsea_persist_")]) == 13


def test_tool_usage_message(tmp_path):
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: fsea-persistence FILE --size N")
    for flag in ("--hop", "--window", "--flip", "--mode db5|db10|db:LO:HI", "--map sat|lin|log", "--full", "--traces", "-o OUT.png"):
        assert flag in r.stdout, flag
    for args, text in (([], "no recording file given"), (["x.raw"], "--size"), (["x.raw", "--size", "0"], "--size"),
                       (["x.raw", "--size", "64", "--hop", "-1"], "--hop"), (["x.raw", "--size", "64", "--map", "cube"], "--map"),
                       (["x.raw", "--size", "64", "--mode", "db7"], "--mode"), (["x.raw", "--size", "64", "--mode", "db:5:5"], "LO < HI"),
                       (["x.raw", "--size", "64", "--bogus"], "usage: fsea-persistence"),
                       ([str(tmp_path / "missing.raw"), "--size", "64"], "cannot open recording")):
        r = subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)


def test_shipped_library_has_the_persistence_kernels_within_their_budget():
    """The add kernels (16-byte and element-wise forms), the image and the decay kernel: wave64, 256 lanes, no scratch, no
    spills, at most 128 VGPRs; the add kernels' histogram is 256 levels x 64 columns of u32 = 64 KiB of static LDS, within
    the 80 KiB that leave two workgroups on a CU's 160 KiB.  u32 counters: no run of rows can overflow one."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    for name, lds in (("fsea_persist_u8", 65536), ("fsea_persist_f32", 65536), ("fsea_persist_u8_narrow", 65536),
                      ("fsea_persist_f32_narrow", 65536), ("fsea_persist_image", 0), ("fsea_persist_decay_u32", 0)):
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] == lds <= 80 * 1024, (name, k[".group_segment_fixed_size"])
    assert 256 * 64 * 4 == 65536 and fsea.PERSIST_RUN_ROWS % 64 == 0


def test_the_column_permutation_puts_a_bank_group_on_32_banks():
    """The arithmetic of DESIGN.md: position(c) = 16 (c & 3) + 4 ((c >> 2) & 3) + (c >> 4), bank = position mod 32.
    u8: lane (s, l), s < 8, l < 4, at step (k, j) counts column 16 l + 4 ((k + s) & 3) + ((j + (s >> 2)) & 3);
    f32: lane (s, m), s < 2, m < 16, at step j counts column 4 m + ((j + s) & 3).  Every step: 32 distinct banks.
    The natural order with a 4-byte load per lane and 16 lanes per row: 4 lanes on each of 8 banks per group."""
    def pos(c):
        return 16 * (c & 3) + 4 * ((c >> 2) & 3) + (c >> 4)

    assert sorted(pos(c) for c in range(64)) == list(range(64)) and all(pos(pos(c)) == c for c in range(64))
    for k in range(4):
        for j in range(4):
            banks = {pos(16 * l + 4 * ((k + s) & 3) + ((j + (s >> 2)) & 3)) % 32 for s in range(8) for l in range(4)}
            assert len(banks) == 32, (k, j)
    for j in range(4):
        assert len({pos(4 * m + ((j + s) & 3)) % 32 for s in range(2) for m in range(16)}) == 32, j
        natural = [(4 * m + j) % 32 for s in range(2) for m in range(16)]
        assert len(set(natural)) == 8 and all(natural.count(b) == 4 for b in set(natural))
