"""GPU tier: the blends of two resident blocks (fsea_interp_*, kernels fsea_interp_frames_* / fsea_interp_image_u8), the
nrf_interpolator block and the fsea-gradual-noise tool on top of them, against the reference's own numbers
(tests/golden/interp_golden.npz) and the numpy restatement of tests/interp_ref.py.  Every output is an integer or a double
produced by the same three rounded operations, so every comparison is exact."""
import ctypes
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import interp_ref as R
from tests.test_interp_host import GOLDEN, TOOL, generator, sha

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def same(got, want):
    """Bit for bit, NaNs included."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def weights_batch():
    ts, _, last = R.pair_weights(0.01)
    return np.array([0.0, 1.0] + ts[1:40:3] + [ts[-1], last, 1.5, -0.25, np.nan, 0.5, 1e300, -1e-300, np.inf], dtype=np.float64)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_nrf_interpolator_equals_the_references(gold, kind):
    gen = generator()
    L = nrf.nrf_lib()
    blocks, length, channels = gen.interp_inputs()[kind]
    new = L.nut_buffer_new_u8 if kind == "u8" else L.nut_buffer_new_f64
    for k, (step, calls) in enumerate(zip(gen.STEPS, gen.CALLS)):
        key = "%s__s%d" % (kind, k)
        recorded = list(gold["buf__%s__calls" % key])
        ip = L.nrf_interpolator_new(step)
        assert ip.contents.t == -1.0 and not ip.contents.buffer_a and not ip.contents.buffer_b
        ts = []
        for i in range(calls):
            b = blocks[i % len(blocks)]
            buf = new(length, channels, b.ctypes.data)
            L.nrf_interpolator_process(ip, buf)
            L.nut_buffer_free(buf)
            ts.append(ip.contents.t)
            if i in recorded:
                j = recorded.index(i)
                got = L.nrf_interpolator_get_buffer(ip)
                c = got.contents
                assert (c.type, c.length, c.channels) == tuple(gold["buf__%s__shape" % key][j])
                a = nrf.buffer_to_numpy(L, got)
                L.nut_buffer_free(got)
                assert np.array_equal(sha(a), gold["buf__%s__sha256" % key][j]), (key, i)
                whole = gold.get("buf__%s__c%d" % (key, i))
                if whole is not None:
                    assert same(a, whole), (key, i)
        L.nrf_interpolator_free(ip)
        assert same(np.array(ts), gold["t__" + key]), key


def test_nrf_interpolator_errors_exit(tmp_path):
    prog = ("import numpy as np\nfrom frequensea_amd import nrf\nL = nrf.nrf_lib()\nip = L.nrf_interpolator_new(1.0)\n%s")
    before = "L.nrf_interpolator_get_buffer(ip)\n"
    other = ("a = L.nut_buffer_new_u8(64, 2, None)\nb = L.nut_buffer_new_u8(32, 2, None)\n"
             "L.nrf_interpolator_process(ip, a)\nL.nrf_interpolator_process(ip, a)\nL.nrf_interpolator_process(ip, b)\n")
    import sys
    from tests.conftest import ROOT
    for body in (before, other):
        r = subprocess.run([sys.executable, "-c", prog % body], capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode == 1 and "NRF interpolator fatal error" in r.stderr, r.stderr[-400:]


SIZES = {"u8": [262144, 4096 * 3 + 5, 4099, 17, 16, 15, 1], "f64": [131072 * 2, 10239, 513, 2, 1]}


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_sample_form_host_and_device(kind):
    rng = np.random.default_rng(5)
    w = weights_batch()
    for n in SIZES[kind]:
        if kind == "u8":
            a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
            a[:4], b[:4] = [0, 255, 127, 128][:min(n, 4)], [255, 0, 128, 127][:min(n, 4)]
        else:
            a, b = rng.standard_normal(n), rng.standard_normal(n) * 1e3
            b[0] = np.nan
        ip = fsea.Interp(a.dtype, n)
        assert same(ip.frames([0.3]), np.zeros((1, n), a.dtype))                 # A and B start as zeros
        ip.push(a)
        assert same(ip.frames(w), R.blend_frames(np.zeros_like(a), a, w)), (kind, n)
        ip.push(b)
        want = R.blend_frames(a, b, w)
        got = ip.frames(w)
        assert same(got, want), (kind, n)
        for f in (0, 5, len(w) - 5, len(w) - 1):                                 # frame f of a batch = a one-frame call
            assert same(ip.frames(w[f:f + 1])[0], got[f])
        assert ip.frames([]).shape == (0, n)
        # device form, on a stream, into a buffer with guard bytes behind it
        d_w, d_out = fsea.DeviceBuffer(w.nbytes).upload(w), fsea.DeviceBuffer(want.nbytes + 64).upload(np.full(want.nbytes + 64, 0xA5, np.uint8))
        ip.frames_device(d_w.ptr, len(w), d_out.ptr)
        fsea._check(ip._L.fsea_interp_frames_device(ip._p, d_w.ptr, 0, None, None))   # n_frames 0: nothing happens
        raw = d_out.download(np.uint8, d_out.nbytes)
        assert raw[:want.nbytes].tobytes() == want.tobytes() and np.all(raw[want.nbytes:] == 0xA5), (kind, n)
        ip.reset()
        assert same(ip.frames([0.7]), np.zeros((1, n), a.dtype))
        d_w.free(), d_out.free(), ip.close()


def test_push_order_on_one_stream_and_two_objects_on_two_streams():
    L = fsea.hip_lib()
    rng = np.random.default_rng(6)
    n, w = 70001, np.array([0.0, 0.25, 1.0, 1.0000000000000007])
    blocks = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(5)]
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        fsea._check(L.fsea_stream_create(0, ctypes.byref(s)))
    objs = [fsea.Interp(np.uint8, n), fsea.Interp(np.uint8, n)]
    d_w = fsea.DeviceBuffer(w.nbytes).upload(w)
    d_blocks = [fsea.DeviceBuffer(n).upload(b) for b in blocks]
    outs = [[fsea.DeviceBuffer(len(w) * n) for _ in blocks] for _ in objs]
    # object 0 takes the blocks in order, object 1 in reverse; pushes and frames alternate without any wait
    order = [list(range(5)), list(range(4, -1, -1))]
    for k in range(5):
        for o, ip in enumerate(objs):
            ip.push_device(d_blocks[order[o][k]].ptr, stream=streams[o])
            ip.frames_device(d_w.ptr, len(w), outs[o][k].ptr, stream=streams[o])
    for ip in objs:
        ip.close()                                             # destroy waits for the device
    for o in range(2):
        for k in range(5):
            a = blocks[order[o][k - 1]] if k else np.zeros(n, np.uint8)
            assert same(outs[o][k].download(np.uint8, outs[o][k].nbytes).reshape(len(w), n), R.blend_frames(a, blocks[order[o][k]], w)), (o, k)
    for b in [d_w] + d_blocks + outs[0] + outs[1]:
        b.free()
    for s in streams:
        fsea._check(L.fsea_stream_destroy(0, s))


def test_image_form_at_the_tools_geometry(gold):
    gen = generator()
    caps = gen.movie_captures()
    ts, eased, _ = R.pair_weights(0.01)
    ip = fsea.Interp(np.uint8, 131072)
    ip.push(caps[0])
    extra = [1.5, -0.5, np.nan, 1.0000000000000007]
    for pair in range(2):
        ip.push(caps[pair + 1])
        w = np.array(eased + extra)
        d_w, d_img = fsea.DeviceBuffer(w.nbytes).upload(w), fsea.DeviceBuffer(len(w) * 1920 * 1080)
        ip.image_frames_device(d_w.ptr, len(w), 1920, 1080, 256, d_img.ptr)
        got = d_img.download(np.uint8, d_img.nbytes).reshape(len(w), 1080, 1920)
        d_w.free(), d_img.free()
        for k in range(100):                                   # the reference binary's own frames
            assert np.array_equal(sha(got[k]), gold["movie__sha256"][100 * pair + k]), (pair, k)
        if pair == 0:
            assert same(got[gen.MOVIE_WHOLE - 1], gold["movie__frame%d" % gen.MOVIE_WHOLE])
        want = R.image_frames(caps[pair], caps[pair + 1], w, 1920, 1080, 256)
        assert same(got, want)
    # the host form, a few frames, without the flip
    w = np.array([0.0, 0.37, 1.0])
    assert same(ip.image_frames(w, 1920, 1080, 256, flip=False), R.image_frames(caps[1], caps[2], w, 1920, 1080, 256, flip=False))
    ip.close()


@pytest.mark.parametrize("width,height,iq_size", [(100, 60, 256), (37, 23, 10), (250, 100, 100), (48, 80, 32), (1, 1, 1),
                                                  (640, 360, 256), (16, 7, 3)])
def test_image_form_odd_geometries(width, height, iq_size):
    rng = np.random.default_rng(7)
    n = 2 * iq_size * iq_size
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    a[0:8:2], b[0:8:2] = np.array([0, 255, 127, 128], np.uint8)[:len(a[0:8:2])], np.array([255, 0, 128, 127], np.uint8)[:len(a[0:8:2])]
    ip = fsea.Interp(np.uint8, n)
    ip.push(a), ip.push(b)
    w = np.concatenate([np.linspace(-0.2, 1.2, 19), [np.nan]])
    want = R.image_frames(a, b, w, width, height, iq_size)
    assert same(ip.image_frames(w, width, height, iq_size), want)
    d_w = fsea.DeviceBuffer(w.nbytes).upload(w)
    d_img = fsea.DeviceBuffer(want.nbytes + 64).upload(np.full(want.nbytes + 64, 0xA5, np.uint8))
    ip.image_frames_device(d_w.ptr, len(w), width, height, iq_size, d_img.ptr)
    raw = d_img.download(np.uint8, d_img.nbytes)
    assert raw[:want.nbytes].tobytes() == want.tobytes() and np.all(raw[want.nbytes:] == 0xA5)
    d_w.free(), d_img.free(), ip.close()


def capture_dir(tmp_path):
    gen = generator()
    caps = gen.movie_captures()
    (tmp_path / "rf").mkdir()
    (tmp_path / "out").mkdir()
    for k, c in enumerate(caps):
        c.tofile(str(tmp_path / "rf" / ("rf-%.3f-big.raw" % (1.0 + 0.01 * k))))
    return caps


def read_png(path):
    L = nrf.nrf_lib()
    L.read_gray_png.restype = ctypes.POINTER(ctypes.c_uint8)
    L.read_gray_png.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    w, h = ctypes.c_int(), ctypes.c_int()
    p = L.read_gray_png(str(path).encode(), ctypes.byref(w), ctypes.byref(h))
    assert p
    return np.ctypeslib.as_array(p, shape=(h.value, w.value)).copy()


def test_tool_raw_and_png(tmp_path, gold):
    capture_dir(tmp_path)
    common = [TOOL, "--dir", str(tmp_path / "rf"), "--out", str(tmp_path / "out")]
    subprocess.run(common + ["--frames", "103", "--raw"], check=True, capture_output=True, timeout=300)
    for no in range(1, 104):                                   # the reference binary's frames, across a swap of pairs
        frame = np.fromfile(str(tmp_path / "out" / ("noise-%d.raw" % no)), dtype=np.uint8)
        assert frame.size == 1920 * 1080 and np.array_equal(sha(frame), gold["movie__sha256"][no - 1]), no
    assert not (tmp_path / "out" / "noise-104.raw").exists()
    subprocess.run(common + ["--frames", "3"], check=True, capture_output=True, timeout=300)
    for no in range(1, 4):
        img = read_png(tmp_path / "out" / ("noise-%d.png" % no))
        assert img.shape == (1080, 1920) and np.array_equal(sha(img), gold["movie__sha256"][no - 1]), no
    # another geometry and step through the arguments
    caps = generator().movie_captures()
    subprocess.run(common + ["--frames", "5", "--raw", "--width", "100", "--height", "60", "--iq-size", "128", "--step", "0.3",
                             "--start", "1.01"], check=True, capture_output=True, timeout=300)
    _, eased, _ = R.pair_weights(0.3)
    assert len(eased) == 4
    want = np.concatenate([R.image_frames(caps[1], caps[2], eased, 100, 60, 128), R.image_frames(caps[2], caps[3], eased[:1], 100, 60, 128)])
    for no in range(1, 6):
        frame = np.fromfile(str(tmp_path / "out" / ("noise-%d.raw" % no)), dtype=np.uint8)
        assert same(frame.reshape(60, 100), want[no - 1]), no


def test_tool_missing_or_short_capture_is_an_error(tmp_path):
    capture_dir(tmp_path)
    common = [TOOL, "--out", str(tmp_path / "out"), "--frames", "2", "--raw"]
    r = subprocess.run(common + ["--dir", str(tmp_path / "nowhere")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cannot open capture" in r.stderr
    r = subprocess.run(common + ["--dir", str(tmp_path / "rf"), "--iq-size", "512"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "bytes" in r.stderr
    assert not list((tmp_path / "out").iterdir())


def test_argument_errors_come_before_device_work():
    L = fsea.hip_lib()
    p = ctypes.c_void_p()
    assert L.fsea_interp_create(None, fsea.IQ_U8, 16, 0) == EINVAL
    assert L.fsea_interp_create(ctypes.byref(p), fsea.IQ_F32, 16, 0) == EINVAL and not p
    assert L.fsea_interp_create(ctypes.byref(p), 7, 16, 0) == EINVAL
    assert L.fsea_interp_create(ctypes.byref(p), fsea.IQ_U8, (1 << 31) + 1, 0) == EINVAL
    assert L.fsea_interp_create(ctypes.byref(p), fsea.IQ_U8, 16, 99) == EINVAL
    assert L.fsea_interp_reset(None) == EINVAL and L.fsea_interp_destroy(None) == 0
    assert L.fsea_interp_push_host(None, None) == EINVAL and L.fsea_interp_push_device(None, None, None) == EINVAL
    ip, f64 = fsea.Interp(np.uint8, 2 * 16 * 16), fsea.Interp(np.float64, 2 * 16 * 16)
    w = np.zeros(4)
    out = np.zeros(4 * 512 + 4096, dtype=np.uint8)
    d = fsea.DeviceBuffer(8192)
    g = fsea.InterpGeometry(32, 32, 16, 1)
    gp = ctypes.byref(g)
    assert L.fsea_interp_push_host(ip._p, None) == EINVAL
    assert L.fsea_interp_push_device(ip._p, None, None) == EINVAL
    assert L.fsea_interp_frames_host(None, w.ctypes.data, 1, out.ctypes.data) == EINVAL
    assert L.fsea_interp_frames_host(ip._p, None, 1, out.ctypes.data) == EINVAL
    assert L.fsea_interp_frames_host(ip._p, w.ctypes.data, 1, None) == EINVAL
    assert L.fsea_interp_frames_host(ip._p, w.ctypes.data, -1, out.ctypes.data) == EINVAL
    assert L.fsea_interp_frames_device(ip._p, d.ptr, 1, None, None) == EINVAL
    assert L.fsea_interp_frames_device(ip._p, None, 1, d.ptr, None) == EINVAL
    assert L.fsea_interp_frames_device(ip._p, d.ptr, 1, d.ptr.value + 8, None) == EINVAL       # misaligned output
    assert L.fsea_interp_frames_device(ip._p, d.ptr.value + 4, 1, d.ptr, None) == EINVAL       # misaligned weights
    assert L.fsea_interp_image_frames_host(ip._p, w.ctypes.data, 1, None, out.ctypes.data) == EINVAL
    assert L.fsea_interp_image_frames_host(f64._p, w.ctypes.data, 1, gp, out.ctypes.data) == EINVAL   # not U8
    assert L.fsea_interp_image_frames_host(ip._p, w.ctypes.data, -1, gp, out.ctypes.data) == EINVAL
    assert L.fsea_interp_image_frames_host(ip._p, None, 1, gp, out.ctypes.data) == EINVAL
    assert L.fsea_interp_image_frames_device(ip._p, d.ptr, 1, gp, d.ptr.value + 8, None) == EINVAL
    for bad in ((0, 32, 16), (32, 0, 16), (32, 32, 0), (16385, 32, 16), (32, 32, 4097), (32, 32, 17)):   # 17: blocks too short
        gb = fsea.InterpGeometry(bad[0], bad[1], bad[2], 1)
        assert L.fsea_interp_image_frames_host(ip._p, w.ctypes.data, 1, ctypes.byref(gb), out.ctypes.data) == EINVAL, bad
    assert not np.any(out)
    assert L.fsea_interp_n_elements(ip._p) == 512 and L.fsea_interp_n_elements(None) == 0
    d.free(), ip.close(), f64.close()
