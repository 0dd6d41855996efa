"""CPU tier: the IQ constellation images' host side -- a numpy restatement of the reference's coordinate rule
(nut_buffer_get_u8), point histogram, draw_line and pixel_inc, checked against tests/golden/iq_draw_golden.npz (recorded
by tests/golden/make_iq_draw_golden.py from the reference's own src/nrf.c); the closed form the line kernel uses, proved
equal to draw_line for every (dx, dy); add_position_channel and the signal detector bit for bit; the argument checks of
fsea_iq_* (before any device work); the fatal-error convention of the nrf calls; the shipped kernels' resources."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

GOLDEN = os.path.join(ROOT, "tests", "golden", "iq_draw_golden.npz")
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_iq_draw_golden.py")
REF_SRC = os.environ.get("FSEA_REFERENCE_SRC", os.path.join(os.path.dirname(ROOT), "reference", "src"))  # as the generator
FSEA_EINVAL = -1
INPUTS = ["block", "filt51", "filt97", "dvbt", "synthetic"]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def iq_inputs():
    """The golden's inputs, rebuilt from committed data exactly as the generator builds them."""
    sys.path.insert(0, os.path.dirname(GENERATOR))
    try:
        import make_iq_draw_golden as g
    finally:
        sys.path.pop(0)
    return g.iq_inputs()


# ---- the restatement ---------------------------------------------------------------------------------------------

def coords(a):
    """nut_buffer_get_u8 on x86-64: u8 as is; a float v -> cvttsd2si(v * 256.0) (0x80000000 for NaN and outside the int32
    range), low byte.  f32 values are widened to f64 first."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.int64)
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * 256.0
        ok = (s > -2147483649.0) & (s < 2147483648.0)
        t = np.trunc(np.where(ok, s, 0.0)).astype(np.int64)
    return np.where(ok, t, 0) & 0xFF


def points_image(a):
    """nrf_buffer_to_iq_points: bin I * 256 + Q, u8++ wrapping; an incomplete last pair is ignored."""
    c = coords(a)
    n = c.size // 2
    return (np.bincount(c[0:2 * n:2] * 256 + c[1:2 * n:2], minlength=65536) % 256).astype(np.uint8)


def line_points(size, pct):
    """The points nrf_buffer_to_iq_lines visits: i = 0, 2, ... < (int)((float)size * clampf(pct, 0, 1))."""
    p = np.float32(pct)
    p = np.float32(0) if p < 0 else np.float32(1) if p > 1 else p
    with np.errstate(invalid="ignore"):
        prod = np.float32(size) * p
    if not prod < np.float32(2 ** 31):
        return 0                                                # x86: (int)NaN = INT_MIN, no point
    mx = int(prod)
    return min((mx + 1) // 2 if mx > 0 else 0, size // 2)


def draw_lines_counts(x1, y1, x2, y2, stride):
    """The reference's draw_line, one iteration of its loop for all segments at once; returns the u32 counts per pixel."""
    x1, y1, x2, y2 = (np.asarray(v, dtype=np.int64).copy() for v in (x1, y1, x2, y2))
    dx, dy = np.abs(x2 - x1), np.abs(y2 - y1)
    sx, sy = np.where(x1 < x2, 1, -1), np.where(y1 < y2, 1, -1)
    err = np.where(dx > dy, dx // 2, -(dy // 2))                # (dx > dy ? dx : -dy) / 2, C truncation
    x, y = x1, y1
    counts = np.zeros(stride * stride, dtype=np.int64)
    while x.size:
        counts += np.bincount(y * stride + x, minlength=stride * stride)
        go = ~((x == x2) & (y == y2))
        x, y, x2, y2, dx, dy, sx, sy, err = (v[go] for v in (x, y, x2, y2, dx, dy, sx, sy, err))
        e2 = err.copy()
        mx, my = e2 > -dx, e2 < dy
        err = err - dy * mx + dx * my
        x = x + sx * mx
        y = y + sy * my
    return counts


def lines_image(a, m, n_points):
    """nrf_buffer_to_iq_lines on the first n_points points: each joined to the next, pixel (I m, Q m) at row Q m,
    pixel_inc saturating at 255."""
    c = coords(a)
    I, Q = c[0:2 * n_points:2] * m, c[1:2 * n_points:2] * m
    counts = draw_lines_counts(I[:-1], Q[:-1], I[1:], Q[1:], 256 * m) if n_points >= 2 else np.zeros((256 * m) ** 2)
    return np.minimum(counts, 255).astype(np.uint8)


def closed_form(x1, y1, x2, y2):
    """The line kernel's pixel t of each segment (csrc/fsea_iq_draw.hip, line_pixel): the major axis moves every step,
    the minor coordinate after t steps is (t d - L / 2 + L - 1) / L.  Returns every segment's pixels (x, y) in order."""
    x1, y1, x2, y2 = (np.asarray(v, dtype=np.int64) for v in (x1, y1, x2, y2))
    dx, dy = np.abs(x2 - x1), np.abs(y2 - y1)
    sx, sy = np.where(x1 < x2, 1, -1), np.where(y1 < y2, 1, -1)
    xmajor = dx > dy
    L, d = np.where(xmajor, dx, dy), np.where(xmajor, dy, dx)
    seg = np.repeat(np.arange(x1.size), L + 1)
    t = np.arange(seg.size) - np.repeat(np.cumsum(L + 1) - (L + 1), L + 1)
    Ls, ds = L[seg], d[seg]
    k = np.where(Ls > 0, (t * ds - Ls // 2 + Ls - 1) // np.maximum(Ls, 1), 0)
    x = x1[seg] + sx[seg] * np.where(xmajor[seg], t, k)
    y = y1[seg] + sy[seg] * np.where(xmajor[seg], k, t)
    return x, y


def sha(img):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(img).tobytes()).digest(), dtype=np.uint8)


# ---- tests --------------------------------------------------------------------------------------------------------

def test_coordinate_rule_is_the_references(gold):
    want = gold["coords__synthetic"]
    assert np.array_equal(coords(gold["in__synthetic"]), want)
    # the contract's examples (x86-64 gcc -O2), and the f32 widening
    v = np.array([-0.01, -0.001, 1.0, 1.004, 1.5, -1.5, np.nan, np.inf, -np.inf, 1e10, -1e10])
    assert coords(v).tolist() == [254, 0, 0, 1, 128, 128, 0, 0, 0, 0, 0]
    f = np.random.default_rng(3).uniform(-4, 4, 4096).astype(np.float32)
    assert np.array_equal(coords(f), coords(f.astype(np.float64)))
    # the reference's own nut_buffer_get_u8, as this library's nut.c compiles it
    L = nrf.nrf_lib()
    a = np.ascontiguousarray(gold["in__synthetic"])
    buf = L.nut_buffer_new_f64(a.size // 2, 2, a.ctypes.data)
    got = np.array([L.nut_buffer_get_u8(buf, i) for i in range(a.size)], dtype=np.uint8)
    L.nut_buffer_free(buf)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", INPUTS)
def test_restatement_equals_the_golden_images(gold, name):
    a = iq_inputs()[name]
    assert np.array_equal(points_image(a), gold["points__" + name])
    cache = {}
    for m in gold["lines__multipliers"]:
        m = int(m)
        for k, p in enumerate(gold["lines__pcts"]):
            n = line_points(a.size, p)
            if (m, n) not in cache:
                cache[(m, n)] = lines_image(a, m, n)
            img = cache[(m, n)]
            key = "lines__%s__m%d__p%d" % (name, m, k)
            assert np.array_equal(sha(img), gold[key + "__sha256"]), key
            assert np.array_equal(img.reshape(256 * m, -1).sum(axis=1, dtype=np.int64), gold[key + "__rowsum"]), key
            if m == 1:
                assert np.array_equal(img, gold[key + "__image"]), key


def test_golden_covers_wrap_saturation_and_empty_images(gold):
    # dvbt: the zero back half lands on bin (0, 0) more than 256 times
    a = iq_inputs()["dvbt"]
    c = coords(a)
    assert np.count_nonzero((c[0::2] == 0) & (c[1::2] == 0)) > 256
    assert gold["points__dvbt"][0] == np.count_nonzero((c[0::2] == 0) & (c[1::2] == 0)) % 256
    # the block's lines at 100 % saturate somewhere; 0 %, a negative and a NaN percentage draw nothing
    assert gold["lines__block__m1__p3__image"].max() == 255
    pcts = list(gold["lines__pcts"])
    for k, p in enumerate(pcts):
        if not p > 0:
            assert not gold["lines__block__m1__p%d__image" % k].any(), p


@pytest.mark.parametrize("m", [1, 4])
def test_closed_form_equals_draw_line_for_every_direction(m):
    """Every (dx, dy) with |dx|, |dy| <= 255 m in steps of m (all four sign combinations), from a start point that keeps
    the segment inside the image."""
    S = 256 * m
    d = np.arange(-255, 256) * m
    DX, DY = np.meshgrid(d, d, indexing="ij")
    DX, DY = DX.ravel(), DY.ravel()
    x1, y1 = np.where(DX < 0, S - 1, 0), np.where(DY < 0, S - 1, 0)
    x2, y2 = x1 + DX, y1 + DY
    xc, yc = closed_form(x1, y1, x2, y2)
    seg = np.repeat(np.arange(x1.size), np.maximum(np.abs(DX), np.abs(DY)) + 1)
    # draw_line's pixels in loop order, with their segment
    xs, ys, ss = [], [], []
    X1, Y1, X2, Y2 = x1.copy(), y1.copy(), x2, y2
    dx, dy = np.abs(X2 - X1), np.abs(Y2 - Y1)
    sx, sy = np.where(X1 < X2, 1, -1), np.where(Y1 < Y2, 1, -1)
    err = np.where(dx > dy, dx // 2, -(dy // 2))
    x, y, sid = X1, Y1, np.arange(x1.size)
    while x.size:
        xs.append(x), ys.append(y), ss.append(sid)
        go = ~((x == X2) & (y == Y2))
        x, y, X2, Y2, dx, dy, sx, sy, err, sid = (v[go] for v in (x, y, X2, Y2, dx, dy, sx, sy, err, sid))
        e2 = err.copy()
        mx, my = e2 > -dx, e2 < dy
        err = err - dy * mx + dx * my
        x, y = x + sx * mx, y + sy * my
    xs, ys, ss = np.concatenate(xs), np.concatenate(ys), np.concatenate(ss)
    # the loop emits step t of every segment in round t: order by (segment, round) = (segment, t)
    order = np.argsort(ss, kind="stable")
    assert np.array_equal(ss[order], seg)
    assert np.array_equal(xs[order], xc) and np.array_equal(ys[order], yc)


def test_position_channel_and_signal_detector_are_the_references(gold):
    L = nrf.nrf_lib()
    a = gold["position__u8_in"]
    buf = L.nut_buffer_new_u8(a.size // 2, 2, a.ctypes.data)
    out = L.nrf_buffer_add_position_channel(buf)
    assert (out.contents.type, out.contents.length, out.contents.channels) == (nrf.NUT_BUFFER_U8, a.size // 2, 3)
    assert np.array_equal(nrf.buffer_to_numpy(L, out), gold["position__u8_out"])
    L.nut_buffer_free(out)
    L.nut_buffer_free(buf)
    f = np.ascontiguousarray(gold["position__f64_in"])
    buf = L.nut_buffer_new_f64(f.size // 3, 3, f.ctypes.data)
    out = L.nrf_buffer_add_position_channel(buf)
    assert (out.contents.type, out.contents.length, out.contents.channels) == (nrf.NUT_BUFFER_F64, f.size // 3, 4)
    assert np.array_equal(nrf.buffer_to_numpy(L, out), gold["position__f64_out"])
    L.nut_buffer_free(out)
    L.nut_buffer_free(buf)
    inputs = iq_inputs()
    for name in ("filt51", "block"):
        a = np.ascontiguousarray(inputs[name])
        buf = (L.nut_buffer_new_u8 if a.dtype == np.uint8 else L.nut_buffer_new_f64)(a.size // 2, 2, a.ctypes.data)
        det = L.nrf_signal_detector_new()
        assert det.contents.mean == 0 and det.contents.standard_deviation == 0
        L.nrf_signal_detector_process(det, buf)
        got = np.array([det.contents.mean, det.contents.standard_deviation])
        L.nrf_signal_detector_free(det)
        L.nut_buffer_free(buf)
        assert np.array_equal(got, gold["detector__" + name]), name


def test_line_points_follow_the_references_float_rule():
    assert line_points(262144, 0.3) == 39322              # (int)(262144 * 0.3f) = 78643 -> i = 0, 2, ..., 78642
    assert line_points(262144, 1.0) == 131072 and line_points(262144, 7.0) == 131072
    assert line_points(262144, 0.0) == 0 and line_points(262144, -1.0) == 0 and line_points(262144, float("nan")) == 0
    assert line_points(7, 1.0) == 3                        # an incomplete last pair is not read


def test_iq_draw_create_needs_a_device():
    """FSEA_ENODEVICE without a GPU (no CPU fallback); with one, a device index out of range is FSEA_EINVAL and a valid one
    creates an object."""
    L = fsea.hip_lib()
    d = ctypes.c_void_p()
    n = fsea.device_count()
    if n < 1:
        assert L.fsea_iq_draw_create(ctypes.byref(d), 0) == -2                  # FSEA_ENODEVICE
        assert not d.value and b"no CPU fallback" in L.fsea_last_error_string()
    else:
        assert L.fsea_iq_draw_create(ctypes.byref(d), n) == FSEA_EINVAL and not d.value
        assert L.fsea_iq_draw_create(ctypes.byref(d), 0) == 0 and d.value
        assert L.fsea_iq_draw_destroy(d) == 0


def test_iq_draw_python_wrapper_rejects_more_points_than_given():
    draw = fsea.IqDraw.__new__(fsea.IqDraw)                # no device: the check comes before the library call
    draw._p = ctypes.c_void_p()
    with pytest.raises(ValueError, match="n_points"):
        draw.lines(np.zeros(8, np.uint8), m=1, n_points=5)
    with pytest.raises(ValueError, match="n_points"):
        draw.lines(np.zeros(8, np.uint8), m=1, n_points=-1)


def test_iq_draw_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    d = ctypes.c_void_p()
    assert L.fsea_iq_draw_create(None, 0) == FSEA_EINVAL
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    assert L.fsea_iq_points_host(None, p, fsea.IQ_U8, 0, 8, p) == FSEA_EINVAL
    assert L.fsea_iq_lines_host(None, p, fsea.IQ_U8, 0, 8, 1, p) == FSEA_EINVAL
    assert L.fsea_iq_points_device(None, p, fsea.IQ_U8, 0, 8, 1, p, None) == FSEA_EINVAL
    assert L.fsea_iq_lines_device(None, p, fsea.IQ_U8, 0, 8, 1, 1, p, None) == FSEA_EINVAL
    assert L.fsea_iq_draw_destroy(None) == 0
    # a non-NULL object that is never dereferenced: every check below fails before the object or a device is used
    fake = ctypes.c_void_p(p)
    for bad_type in (-1, 3, 7):
        assert L.fsea_iq_points_host(fake, p, bad_type, 0, 8, p) == FSEA_EINVAL
        assert L.fsea_iq_lines_device(fake, p, bad_type, 0, 8, 1, 1, p, None) == FSEA_EINVAL
    assert b"type" in L.fsea_last_error_string()
    for m in (0, -1, fsea.IQ_MAX_MULTIPLIER + 1):
        assert L.fsea_iq_lines_host(fake, p, fsea.IQ_U8, 0, 8, m, p) == FSEA_EINVAL
        assert L.fsea_iq_lines_device(fake, p, fsea.IQ_U8, 0, 8, 1, m, p, None) == FSEA_EINVAL
    assert b"size_multiplier" in L.fsea_last_error_string()
    assert L.fsea_iq_points_host(fake, None, fsea.IQ_U8, 0, 8, p) == FSEA_EINVAL
    assert L.fsea_iq_points_host(fake, p, fsea.IQ_U8, 0, 8, None) == FSEA_EINVAL
    assert L.fsea_iq_lines_host(fake, None, fsea.IQ_F64, 0, 8, 2, p) == FSEA_EINVAL
    assert L.fsea_iq_points_device(fake, None, fsea.IQ_U8, 0, 8, 1, p, None) == FSEA_EINVAL
    assert L.fsea_iq_lines_device(fake, p, fsea.IQ_U8, 0, 8, 1, 1, None, None) == FSEA_EINVAL
    assert L.fsea_iq_points_device(fake, p + 1, fsea.IQ_U8, 0, 8, 1, p, None) == FSEA_EINVAL    # alignment
    assert L.fsea_iq_points_device(fake, p, fsea.IQ_U8, 0, 8, -1, p, None) == FSEA_EINVAL      # n_frames
    assert L.fsea_iq_points_host(fake, p, fsea.IQ_U8, 0, (1 << 31) + 1, p) == FSEA_EINVAL      # pairs per frame
    assert not d.value


@pytest.mark.parametrize("call", ["nrf_buffer_to_iq_lines(buf, %d, 0.5)", "nrf_device_get_iq_lines(dev, %d, 0.5)"])
@pytest.mark.parametrize("m", [0, -2, 17])
def test_nrf_iq_lines_with_a_bad_size_multiplier_exits(call, m):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n"
            "buf = L.nut_buffer_new_u8(16, 2, None)\n"
            "dev = L.nrf_device_new(100.0, b'/nonexistent/capture.raw')\n"
            "L.%s\n"
            "print('returned')\n") % (ROOT, call % m)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "size_multiplier %d is outside [1, 16]" % m in r.stderr


def test_nrf_exports_the_iq_drawing_functions():
    syms = subprocess.run(["nm", "-D", "--defined-only", nrf.lib_path()], capture_output=True, text=True,
                          check=True).stdout.split()
    for name in ("nrf_device_get_iq_buffer", "nrf_device_get_iq_lines", "nrf_buffer_add_position_channel",
                 "nrf_buffer_to_iq_points", "nrf_buffer_to_iq_lines", "nrf_signal_detector_new",
                 "nrf_signal_detector_process", "nrf_signal_detector_free"):
        assert name in syms and name in nrf.NRF_EXPORTS, name
    text = open(os.path.join(ROOT, "include", "nrf.h")).read()
    assert re.search(r"typedef struct \{\s*double mean;\s*double standard_deviation;\s*\} nrf_signal_detector;", text)
    assert ctypes.sizeof(nrf.NrfSignalDetector) == 16


def test_shipped_library_has_the_iq_kernels_without_spills():
    if not os.path.exists(LIB):
        pytest.skip("libfsea_hip.so not built")
    ks = _kernels(LIB)
    names = sorted(k for k in ks if k.startswith("fsea_iq_"))
    assert names == ["fsea_iq_clamp", "fsea_iq_lines_f32", "fsea_iq_lines_f64", "fsea_iq_lines_u8",
                     "fsea_iq_points_f32", "fsea_iq_points_f64", "fsea_iq_points_u8"]
    for name in names:
        k = ks[name]
        assert k[".wavefront_size"] == 64, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        if name.startswith("fsea_iq_points"):
            # one workgroup of 1024 lanes per CU, half of the 256 x 256 u32 bins in LDS
            assert k[".max_flat_workgroup_size"] == 1024 and k[".group_segment_fixed_size"] == 128 * 1024, name
            assert k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        else:
            assert k[".max_flat_workgroup_size"] == 256 and k[".group_segment_fixed_size"] == 0, name


@pytest.mark.skipif(not os.path.exists(os.path.join(REF_SRC, "nrf.c")), reason="reference tree absent")
def test_golden_generator_reproduces_the_committed_file(tmp_path, gold):
    out = tmp_path / "iq_draw_golden.npz"
    subprocess.run([sys.executable, GENERATOR, str(out)], check=True, capture_output=True, timeout=600)
    with np.load(out) as z:
        again = {k: z[k] for k in z.files}
    assert sorted(again) == sorted(gold)
    for k in gold:
        assert again[k].dtype == gold[k].dtype and np.array_equal(again[k], gold[k], equal_nan=gold[k].dtype.kind == "f"), k
