"""GPU tier: the IQ trace movie (fsea_trace_*, kernels fsea_trace_hits_* / fsea_trace_compose_*) and the fsea-single-sample
tool on top of it, against the reference binary's own frames (tests/golden/trace_golden.npz) and the numpy restatement of
tests/trace_ref.py.  Every frame is integer arithmetic on bytes, so every comparison is byte for byte."""
import ctypes
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import trace_ref as R
from tests.test_gpu_interp import read_png
from tests.test_trace_host import GOLDEN, TOOL, check_case, generator, sha

pytestmark = pytest.mark.gpu
W, H = 1920, 1080


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def device_frames(tr, data, s, n, images=True, guard=64, stream=0):
    """n frames through the device form in one call: (frames, guard bytes behind them)."""
    d_in = fsea.DeviceBuffer(data.size).upload(data)
    size = n * tr.width * tr.height
    d_out = fsea.DeviceBuffer(size + guard).upload(np.full(size + guard, 0xA5, np.uint8)) if images else None
    tr.frames_device(d_in.ptr, data.size, s, n, d_out.ptr if images else 0, stream=stream)
    if not images:
        tr.canvas()                                        # waits for the launches
        d_in.free()
        return None, None
    raw = d_out.download(np.uint8, d_out.nbytes)
    d_in.free(), d_out.free()
    return raw[:size].reshape(n, tr.height, tr.width), raw[size:]


@pytest.mark.parametrize("name", ["defaults", "fade", "two", "preview", "odd"])
def test_device_form_equals_the_reference_binary(gold, name):
    gen = generator()
    inp, s, f, p, preview, _, _ = gen.CASES[name]
    data = gen.inputs()[inp]
    n = R.n_frames_of(data.size, s)
    tr = fsea.Trace(pixel_inc=p, fade=f)
    if preview:
        device_frames(tr, data, s, n, images=False)
        check_case(gold, name, [tr.canvas()])
    else:
        frames, guard = device_frames(tr, data, s, n)
        check_case(gold, name, frames)
        assert np.all(guard == 0xA5)
        assert same(tr.canvas(), frames[-1])
    tr.close()


def crossing_bytes(n):
    """Two points over and over: every segment of a frame hits the same pixels."""
    return np.tile(np.array([10, 20, 200, 180], np.uint8), -(-n // 4))[:n]


# (width, height, m, pixel_inc, fade, frame_bytes, frames, what it is there for)
GEOMETRIES = [
    (300, 270, 1, 60, 2, 50, 9, "a width that is no multiple of 16, frames that start at every alignment"),
    (256, 256, 1, 254, 0, 34, 9, "256 m == width: the x == width - 1 column is skipped"),
    (523, 517, 2, 1, 255, 2, 5, "two bytes per frame: no segment"),
    (640, 528, 2, 9, 4, 101, 11, "an odd frame size on the aligned kernels"),
    (1040, 1030, 4, 30, 0, 700, 5, "u32 counts, a margin that is no multiple of 16"),
    (270, 300, 1, 100, 10, 64, 9, "byte counts on the unaligned kernels"),
    (1920, 1080, 4, 1, 0, 1500, 3, "749 segments on the same pixels: byte-wide counts would overflow"),
]


@pytest.mark.parametrize("width,height,m,p,f,s,n,why", GEOMETRIES)
def test_restatement_on_other_geometries(width, height, m, p, f, s, n, why):
    rng = np.random.default_rng(width + s)
    data = crossing_bytes(n * s + 3) if s == 1500 else rng.integers(0, 256, n * s + 3, dtype=np.uint8)
    data[0:4] = [128, 128, 127, 127]                       # from (0, 0) to (255, 255)
    want, canvas = R.frames(data, s, n, width, height, m, p, f)
    if s == 1500:
        assert want.max() == 254                           # 749 hits of 1: more than a byte counts, all but 254 refused
    tr = fsea.Trace(width, height, m, p, f)
    got, guard = device_frames(tr, data, s, n)
    assert same(got, want), why
    assert np.all(guard == 0xA5), why
    assert same(tr.canvas(), canvas)
    tr.reset()
    assert not tr.canvas().any()
    assert same(tr.frames(data, s, n), want), why          # the host form, from a zero canvas again
    assert tr.frames(data, s, 0).shape == (0, height, width)
    tr.close()


def test_chunks_of_any_size_give_the_same_frames():
    gen = generator()
    data = gen.inputs()["long_odd"]
    s, n = 333, 48
    one = fsea.Trace(pixel_inc=40, fade=3)
    want = one.frames(data, s, n)
    assert same(want, R.frames(data, s, n, p=40, f=3)[0])
    for step in (1, 7):
        tr = fsea.Trace(pixel_inc=40, fade=3)
        got = np.concatenate([tr.frames(data[f0 * s:], s, min(step, n - f0)) for f0 in range(0, n, step)])
        assert same(got, want), step
        assert same(tr.canvas(), one.canvas()), step
        tr.close()
    one.close()


def test_reset_and_advance_only():
    gen = generator()
    data = gen.inputs()["long"]
    tr = fsea.Trace(pixel_inc=40, fade=3)
    assert not tr.canvas().any()                           # zero after create
    want, canvas = R.frames(data, 1024, 16, p=40, f=3)
    assert tr.frames(data[:6 * 1024], 1024, 6, images=False) is None
    assert same(tr.canvas(), want[5])
    assert same(tr.frames(data[6 * 1024:], 1024, 10), want[6:])     # frames behind an advance-only call
    tr.reset()
    assert not tr.canvas().any()
    assert same(tr.frames(data, 1024, 16), want)
    # frames behind the end of the data only fade
    more = tr.frames(np.zeros(0, np.uint8), 1024, 2)
    assert same(more[1], np.maximum(canvas.astype(np.int64) - 6, 0).astype(np.uint8))
    tr.close()


def test_two_objects_on_two_streams():
    L = fsea.hip_lib()
    gen = generator()
    data = gen.inputs()["long"]
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for st in streams:
        fsea._check(L.fsea_stream_create(0, ctypes.byref(st)))
    cfg = [(40, 3, 1024), (100, 0, 4096)]
    objs = [fsea.Trace(pixel_inc=p, fade=f) for p, f, _ in cfg]
    d_in = fsea.DeviceBuffer(data.size).upload(data)
    calls = 4
    outs = [[fsea.DeviceBuffer((16384 // s // calls) * W * H) for _ in range(calls)] for _, _, s in cfg]
    # every object takes its capture in four calls, the two alternating without any wait
    for c in range(calls):
        for o, (_, _, s) in enumerate(cfg):
            nf = 16384 // s // calls
            first = c * nf * s
            objs[o].frames_device(d_in.ptr.value + first, data.size - first, s, nf, outs[o][c].ptr, stream=streams[o])
    for tr in objs:
        tr.close()                                         # destroy waits for the device
    for o, (p, f, s) in enumerate(cfg):
        nf = 16384 // s // calls
        want = R.frames(data, s, 16384 // s, p=p, f=f)[0]
        for c in range(calls):
            assert same(outs[o][c].download(np.uint8, outs[o][c].nbytes).reshape(nf, H, W), want[c * nf:(c + 1) * nf]), (o, c)
    for b in [d_in] + outs[0] + outs[1]:
        b.free()
    for st in streams:
        fsea._check(L.fsea_stream_destroy(0, st))


def run_tool(tmp_path, data, args, timeout):
    """One run of the tool on `data` into a directory of its own."""
    cap = tmp_path / "capture.raw"
    data.tofile(str(cap))
    out = tmp_path / ("out%d" % len(list(tmp_path.iterdir())))
    out.mkdir()
    subprocess.run([TOOL, "--out", str(out)] + args + [str(cap)], check=True, capture_output=True, timeout=timeout)
    return out


def test_tool_raw_and_png(tmp_path, gold):
    gen = generator()
    data = gen.inputs()
    # 40 frames of 2 MB through files: a minute is generous
    out = run_tool(tmp_path, data["block"], ["--raw", "--frames", "40"], 300)
    for no in range(1, 41):
        frame = np.fromfile(str(out / ("sample-%d.raw" % no)), dtype=np.uint8)
        assert frame.size == W * H and np.array_equal(sha(frame), gold["defaults__sha256"][no - 1]), no
    assert not (out / "sample-41.raw").exists()
    out = run_tool(tmp_path, data["long"], ["-s", "1024", "-f", "3", "-p", "40"], 300)
    for no in range(1, 17):
        img = read_png(out / ("sample-%d.png" % no))
        assert img.shape == (H, W) and np.array_equal(sha(img), gold["fade__sha256"][no - 1]), no
    assert not (out / "sample-17.png").exists()


def test_tool_preview(tmp_path, gold):
    data = generator().inputs()["long"]
    out = run_tool(tmp_path, data, ["-s", "1024", "-f", "3", "-p", "40", "-v"], 300)
    assert [p.name for p in out.iterdir()] == ["sample-17.png"]          # the reference's name: frames + 1
    assert np.array_equal(sha(read_png(out / "sample-17.png")), gold["preview__sha256"][0])


def test_tool_ragged_tail_and_other_geometry(tmp_path, gold):
    data = generator().inputs()
    # an odd step whose last frame ends with half a point, at the tool's geometry
    out = run_tool(tmp_path, data["long_odd"], ["-s", "333", "-f", "1", "-p", "30", "--raw"], 300)
    want = R.frames(data["long_odd"], 333, 48, p=30, f=1)[0]
    for no in range(1, 49):
        frame = np.fromfile(str(out / ("sample-%d.raw" % no)), dtype=np.uint8)
        assert same(frame.reshape(H, W), want[no - 1]), no
        if no < 48:
            assert np.array_equal(sha(frame), gold["odd__sha256"][no - 1]), no
    # a size that is no multiple of the step, a smaller canvas
    tail = data["long"][:5000]
    out = run_tool(tmp_path, tail, ["-s", "1024", "-p", "25", "-f", "2", "--raw", "--width", "600", "--height", "520",
                                    "--multiplier", "2"], 300)
    want = R.frames(tail, 1024, 5, 600, 520, 2, 25, 2)[0]
    for no in range(1, 6):
        frame = np.fromfile(str(out / ("sample-%d.raw" % no)), dtype=np.uint8)
        assert same(frame.reshape(520, 600), want[no - 1]), no
    assert not (out / "sample-6.raw").exists()
