"""GPU tier: the IQ constellation images (fsea_iq_*, kernels fsea_iq_points_* / fsea_iq_lines_* / fsea_iq_clamp) and the
nrf_* drawing functions on top of them, byte for byte against the reference's own images (tests/golden/iq_draw_golden.npz)
and the numpy restatement of tests/test_iq_draw_host.py.  Every image is integer counts, so every comparison is exact."""
import ctypes
import threading
import time

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests.test_iq_draw_host import (GOLDEN, INPUTS, coords, iq_inputs, line_points, lines_image, points_image, sha)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def draw():
    d = fsea.IqDraw()
    yield d
    d.close()


def nut(L, a, channels=2):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return L.nut_buffer_new_u8(a.size // channels, channels, a.ctypes.data)
    return L.nut_buffer_new_f64(a.size // channels, channels, a.ctypes.data)


def take(L, buf):
    out = nrf.buffer_to_numpy(L, buf)
    c = buf.contents
    meta = (c.type, c.length, c.channels)
    L.nut_buffer_free(buf)
    return out, meta


DeviceBuffer = fsea.DeviceBuffer


@pytest.mark.parametrize("name", INPUTS)
def test_nrf_images_equal_the_references(gold, name):
    L = nrf.nrf_lib()
    a = iq_inputs()[name]
    buf = nut(L, a)
    img, meta = take(L, L.nrf_buffer_to_iq_points(buf))
    assert meta == (nrf.NUT_BUFFER_U8, 65536, 1)
    assert np.array_equal(img, gold["points__" + name])
    for m in gold["lines__multipliers"]:
        m = int(m)
        for k, p in enumerate(gold["lines__pcts"]):
            img, meta = take(L, L.nrf_buffer_to_iq_lines(buf, m, float(p)))
            key = "lines__%s__m%d__p%d" % (name, m, k)
            assert meta == (nrf.NUT_BUFFER_U8, (256 * m) ** 2, 1), key
            assert np.array_equal(sha(img), gold[key + "__sha256"]), key
            if m == 1:
                assert np.array_equal(img, gold[key + "__image"]), key
    L.nut_buffer_free(buf)


def test_nrf_device_forms_on_a_paused_stepped_replay_device(gold, tmp_path):
    import importlib.util
    import tests.test_iq_draw_host as host
    spec = importlib.util.spec_from_file_location("gen", host.GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    L = nrf.nrf_lib()
    path = str(tmp_path / "replay.raw")
    blocks = gen.replay_file(path) ^ np.uint8(0x80)
    dev = L.nrf_device_new(100.0, path.encode())
    try:
        L.nrf_device_set_paused(dev, 1)
        seen = set()
        for step in range(4):
            time.sleep(0.1)
            s, _ = take(L, L.nrf_device_get_samples_buffer(dev))
            b = [i for i in range(3) if np.array_equal(s, blocks[i])]
            assert len(b) == 1, step
            b = b[0]
            seen.add(b)
            pts, meta = take(L, L.nrf_device_get_iq_buffer(dev))
            assert meta == (nrf.NUT_BUFFER_U8, 65536, 1)
            assert np.array_equal(pts, gold["device__points"][b]), (step, b)
            img, meta = take(L, L.nrf_device_get_iq_lines(dev, gen.DEVICE_M, gen.DEVICE_PCT))
            assert meta == (nrf.NUT_BUFFER_U8, (256 * gen.DEVICE_M) ** 2, 1)
            assert np.array_equal(sha(img), gold["device__lines_sha256"][b]), (step, b)
            L.nrf_device_step(dev)
        assert seen == {0, 1, 2}
    finally:
        L.nrf_device_free(dev)


@pytest.mark.parametrize("m", [1, 4])
def test_every_direction_against_the_restatement(draw, m):
    """(128, 128) alternating with every (I, Q): segments in all octants, of every length, and zero-length ones."""
    I, Q = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    pts = np.stack([np.full(65536, 128), I.ravel(), np.full(65536, 128), Q.ravel()], axis=1)
    iq = pts[:, [0, 2, 1, 3]].reshape(-1).astype(np.uint8)      # (128, 128), (I, Q), (128, 128), ...
    want = lines_image(iq, m, iq.size // 2)
    got = draw.lines(iq, m=m)
    assert np.array_equal(got.ravel(), want)
    # the same points as f64 (k + 0.5) / 256 and as f32: the same coordinates
    f = (iq.astype(np.float64) + 0.5) / 256.0
    assert np.array_equal(draw.lines(f, m=m).ravel(), want)
    assert np.array_equal(draw.lines(f.astype(np.float32), m=m).ravel(), want)
    assert np.array_equal(draw.points(iq).ravel(), points_image(iq))


def test_points_wrap_and_lines_saturate(draw):
    for n, bin_count in ((131072, 0), (131072 + 300, 44), (1000, 232)):
        iq = np.tile(np.array([17, 200], np.uint8), n)
        img = draw.points(iq)
        assert img[17, 200] == bin_count and np.count_nonzero(img) == (1 if bin_count else 0), n
    # a segment drawn back and forth 200 times: interior pixels get 2 per pass, endpoints more -> 255
    iq = np.tile(np.array([10, 10, 20, 15], np.uint8), 200)
    img = draw.lines(iq, m=1).astype(np.int64)
    assert img.max() == 255 and img[10, 10] == 255 and img[15, 20] == 255
    assert np.array_equal(img.ravel(), lines_image(iq, 1, iq.size // 2))
    counts = lines_image(iq[:4], 1, 2)                            # one segment: each pixel once
    assert counts.sum() == 11 and counts.max() == 1


def test_lines_are_transposed_relative_to_points(draw):
    iq = np.array([10, 200, 10, 200], np.uint8)                  # one zero-length segment at (I, Q) = (10, 200)
    pts = draw.points(iq)
    assert pts[10, 200] == 2 and np.count_nonzero(pts) == 1      # row I
    for m in (1, 2, 4):
        img = draw.lines(iq, m=m)
        assert img[200 * m, 10 * m] == 1 and np.count_nonzero(img) == 1, m   # row Q m, column I m


def test_out_of_range_and_nan_inputs(draw, gold):
    a = gold["in__synthetic"]
    c = coords(a)
    assert np.array_equal(c, gold["coords__synthetic"])
    assert np.array_equal(draw.points(a).ravel(), gold["points__synthetic"])
    with np.errstate(over="ignore"):
        f32 = a.astype(np.float32)                               # f32: the coordinate of the exact widening
    assert np.array_equal(draw.points(f32).ravel(), points_image(f32.astype(np.float64)))
    for m in (1, 2):
        assert np.array_equal(draw.lines(a, m=m).ravel(), lines_image(a, m, a.size // 2)), m
        assert np.array_equal(draw.lines(f32, m=m).ravel(), lines_image(f32.astype(np.float64), m, a.size // 2)), m
    # a NaN percentage through the nrf call draws nothing
    L = nrf.nrf_lib()
    buf = nut(L, a)
    img, _ = take(L, L.nrf_buffer_to_iq_lines(buf, 2, float("nan")))
    L.nut_buffer_free(buf)
    assert not img.any()


@pytest.mark.parametrize("length", [51, 97])
def test_device_chain_fir_into_lines_equals_the_nrf_chain(length):
    """fsea_fir_u8_device -> f32 on the device -> fsea_iq_lines_device equals nrf_iq_filter_get_buffer (f32 widened to
    f64) -> nrf_buffer_to_iq_lines, bit for bit."""
    import os
    from tests.conftest import ROOT
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        block = np.ascontiguousarray(z["block__raw"])            # raw int8 bytes: the device path flips, nrf gets ^ 0x80
    n = block.size // 2
    m, pct = 4, 0.3
    L = nrf.nrf_lib()
    flt = L.nrf_iq_filter_new(5000000, 200000, length)
    buf = nut(L, block ^ 0x80)
    L.nrf_iq_filter_process(flt, buf)
    fb = L.nrf_iq_filter_get_buffer(flt)
    want, _ = take(L, L.nrf_buffer_to_iq_lines(fb, m, pct))
    L.nut_buffer_free(fb)
    L.nut_buffer_free(buf)
    L.nrf_iq_filter_free(flt)

    fir = fsea.Fir(fsea.lowpass_taps(5000000, 200000, length))
    draw = fsea.IqDraw()
    d_in, d_f, d_img = DeviceBuffer(block.nbytes).upload(block), DeviceBuffer(8 * n), DeviceBuffer((256 * m) ** 2)
    fir.run_device(d_in.ptr.value, n, d_f.ptr.value, flip=True)
    draw.lines_device(d_f.ptr.value, fsea.IQ_F32, line_points(2 * n, pct), 1, m, d_img.ptr.value)
    got = d_img.download(np.uint8, d_img.nbytes)
    for b in (d_in, d_f, d_img):
        b.free()
    fir.close()
    draw.close()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("kind", [fsea.IQ_U8, fsea.IQ_F32, fsea.IQ_F64])
def test_batched_device_forms_equal_per_frame_calls(draw, kind):
    rng = np.random.default_rng(10 + kind)
    dtype = {fsea.IQ_U8: np.uint8, fsea.IQ_F32: np.float32, fsea.IQ_F64: np.float64}[kind]
    for n_frames, n in ((1, 4099), (3, 1003), (7, 8192), (5, 2)):
        if kind == fsea.IQ_U8:
            iq = rng.integers(0, 256, 2 * n * n_frames, dtype=np.uint8)
        else:
            iq = rng.uniform(-0.2, 1.2, 2 * n * n_frames).astype(dtype)
        frames = iq.reshape(n_frames, -1)
        d_in = DeviceBuffer(iq.nbytes).upload(iq)
        d_pts = DeviceBuffer(65536 * n_frames)
        draw.points_device(d_in.ptr.value, kind, n, n_frames, d_pts.ptr.value)
        got = d_pts.download(np.uint8, (n_frames, 256, 256))
        for f in range(n_frames):
            assert np.array_equal(got[f], draw.points(frames[f])), (n_frames, n, f)
        m = 2
        d_lines = DeviceBuffer((256 * m) ** 2 * n_frames)
        draw.lines_device(d_in.ptr.value, kind, n, n_frames, m, d_lines.ptr.value)
        got = d_lines.download(np.uint8, (n_frames, 256 * m, 256 * m))
        for f in range(n_frames):
            assert np.array_equal(got[f], draw.lines(frames[f], m=m)), (n_frames, n, f)
        for b in (d_in, d_pts, d_lines):
            b.free()
    # the flip of raw HackRF bytes
    iq = rng.integers(0, 256, 2 * 5000, dtype=np.uint8)
    assert np.array_equal(draw.points(iq, flip=True), draw.points(iq ^ 0x80))
    assert np.array_equal(draw.lines(iq, m=2, flip=True), draw.lines(iq ^ 0x80, m=2))


def test_two_runs_are_identical(draw):
    iq = np.random.default_rng(5).integers(0, 256, 2 * 131072, dtype=np.uint8)
    a, b = draw.lines(iq, m=4), draw.lines(iq, m=4)
    assert np.array_equal(a, b) and a.any()
    assert np.array_equal(draw.points(iq), draw.points(iq))


def test_host_forms_grow_their_staging_and_reuse_it():
    """A fresh object's host forms on a small input, a larger one (more pairs in, a (256 * 4)^2 image out), then small and
    empty ones again: the staging grows on the second call and the later calls run in the larger buffers."""
    d = fsea.IqDraw()
    rng = np.random.default_rng(11)
    for n, m in ((10, 1), (20000, 4), (10, 1), (0, 2)):
        iq = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        assert np.array_equal(d.points(iq).ravel(), points_image(iq)), n
        assert np.array_equal(d.lines(iq, m=m).ravel(), lines_image(iq, m, n)), (n, m)
    d.close()


def test_two_threads_drawing_at_once_get_their_own_images():
    L = nrf.nrf_lib()
    rng = np.random.default_rng(9)
    inputs = [rng.integers(0, 256, 2 * 20000, dtype=np.uint8), rng.uniform(0, 1, 2 * 20000)]
    wants = [(points_image(a), lines_image(a, 2, line_points(a.size, 0.5))) for a in inputs]
    errors = []

    def worker(i):
        try:
            buf = nut(L, inputs[i])
            for _ in range(10):
                p, _ = take(L, L.nrf_buffer_to_iq_points(buf))
                q, _ = take(L, L.nrf_buffer_to_iq_lines(buf, 2, 0.5))
                if not (np.array_equal(p, wants[i][0]) and np.array_equal(q, wants[i][1])):
                    errors.append(i)
            L.nut_buffer_free(buf)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
