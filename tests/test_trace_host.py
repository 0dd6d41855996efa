"""CPU tier of the IQ trace movie: the numpy restatements of tests/trace_ref.py (the literal loop and the order-free form)
against each other and against tests/golden/trace_golden.npz (recorded from a build of the reference's own
c/single-sample.c), the argument checks of fsea_trace_* and of fsea-single-sample (before any device work), and the shipped
kernels' resources.  Nothing here needs a GPU."""
import ctypes
import hashlib
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import trace_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

GOLDEN = os.path.join(ROOT, "tests", "golden", "trace_golden.npz")
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-single-sample")
EINVAL, ENODEVICE = -1, -2
W, H = 1920, 1080


def generator():
    spec = importlib.util.spec_from_file_location("make_trace_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_trace_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def compared_frames(name, n):
    """Every frame, but the last of the odd case (the reference takes that frame's last byte from behind its buffer)."""
    return n - 1 if name == "odd" else n


def check_case(golden, name, frames):
    """frames: what some implementation gives for every frame of the case (for the preview: the final image alone)."""
    want = golden[name + "__sha256"]
    for k in range(compared_frames(name, len(want))):
        assert np.array_equal(sha(frames[k]), want[k]), (name, k + 1)
    for j, no in enumerate(golden[name + "__sums_of"]):
        assert np.array_equal(frames[no - 1].astype(np.int64).sum(axis=1), golden[name + "__rowsum"][j]), (name, no)
        assert np.array_equal(frames[no - 1].astype(np.int64).sum(axis=0), golden[name + "__colsum"][j]), (name, no)
    for key in golden:
        if key.startswith(name + "__frame"):
            no = int(key[len(name + "__frame"):])
            assert np.array_equal(frames[no - 1], golden[key]), key


@pytest.mark.parametrize("name", ["defaults", "fade", "two", "preview", "odd"])
def test_order_free_restatement_matches_the_reference_binary(golden, name):
    gen = generator()
    inp, s, f, p, preview, _, _ = gen.CASES[name]
    assert list(golden[name + "__args"]) == [s, f, p, int(preview)]
    data = gen.inputs()[inp]
    n = R.n_frames_of(data.size, s)
    frames, canvas = R.frames(data, s, n, p=p, f=f)
    assert np.array_equal(canvas, frames[-1])
    if preview:
        assert len(golden[name + "__sha256"]) == 1
        check_case(golden, name, [canvas])
    else:
        assert len(golden[name + "__sha256"]) == n
        check_case(golden, name, frames)
    if name in ("fade", "two"):
        # saturation is reached: some hit was refused
        assert int(frames.max()) + p >= 255
    if name == "fade":
        # the quirk: nothing is drawn where an IQ-square coordinate is 0, and lines do end there
        side, ox, oy = R.geometry(W, H, 4)
        assert not frames[:, oy, :].any() and not frames[:, :, ox].any()
        xs, ys = R.frame_points(data, 0, s)
        assert (xs == 0).any() and (ys == 0).any()


@pytest.mark.parametrize("name,n", [("defaults", 8), ("fade", 1), ("odd", 3)])
def test_literal_loop_equals_the_order_free_form_and_the_reference(golden, name, n):
    gen = generator()
    inp, s, f, p, _, _, _ = gen.CASES[name]
    data = gen.inputs()[inp]
    lit, lit_canvas = R.literal_frames(data, s, n, p=p, f=f)
    free, free_canvas = R.frames(data, s, n, p=p, f=f)
    assert np.array_equal(lit, free) and np.array_equal(lit_canvas, free_canvas)
    for k in range(n):
        assert np.array_equal(sha(lit[k]), golden[name + "__sha256"][k]), (name, k + 1)


def test_restatement_small_geometry_and_chunks():
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, 700, dtype=np.uint8)
    for (w, h, m, p, f, s) in ((300, 256, 1, 60, 2, 50), (256, 256, 1, 254, 0, 33), (523, 517, 2, 1, 255, 2)):
        n = R.n_frames_of(data.size, s)
        lit, _ = R.literal_frames(data, s, n, w, h, m, p, f)
        free, canvas = R.frames(data, s, n, w, h, m, p, f)
        assert np.array_equal(lit, free), (w, h, m, p, f, s)
        # in two calls, the canvas carried
        a, c = R.frames(data, s, 5, w, h, m, p, f)
        b, c = R.frames(data[5 * s:], s, n - 5, w, h, m, p, f, canvas=c)
        assert np.array_equal(np.concatenate([a, b]), free) and np.array_equal(c, canvas)


def test_trace_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    t = ctypes.c_void_p()
    ok = fsea.TraceConfig(1920, 1080, 4, 4, 0)
    assert L.fsea_trace_create(None, ctypes.byref(ok), 0) == EINVAL
    assert L.fsea_trace_create(ctypes.byref(t), None, 0) == EINVAL
    bad = [(1023, 1080, 4, 4, 0), (1920, 1023, 4, 4, 0), (255, 255, 1, 4, 0), (1920, 1080, 0, 4, 0), (1920, 1080, -1, 4, 0),
           (16384, 16384, fsea.IQ_MAX_MULTIPLIER + 1, 4, 0), (16385, 1080, 4, 4, 0), (1920, 1080, 4, 0, 0),
           (1920, 1080, 4, 255, 0), (1920, 1080, 4, -3, 0), (1920, 1080, 4, 4, -1), (1920, 1080, 4, 4, 256)]
    for cfg in bad:
        assert L.fsea_trace_create(ctypes.byref(t), ctypes.byref(fsea.TraceConfig(*cfg)), 0) == EINVAL, cfg
        assert not t.value
    assert b"fade" in L.fsea_last_error_string()
    assert L.fsea_trace_destroy(None) == 0 and L.fsea_trace_reset(None) == EINVAL
    buf = np.zeros(1 << 12, np.uint8)
    p = buf.ctypes.data
    assert L.fsea_trace_frames_host(None, p, 64, 1, 16, 1, p) == EINVAL
    assert L.fsea_trace_frames_device(None, p, 64, 1, 16, 1, p, None) == EINVAL
    assert L.fsea_trace_canvas_host(None, p) == EINVAL
    # a non-NULL object that is never dereferenced: every check below fails before the object or a device is used
    fake = ctypes.c_void_p(p)
    assert L.fsea_trace_frames_host(fake, p, 64, 1, 0, 1, p) == EINVAL                      # frame_bytes
    assert L.fsea_trace_frames_device(fake, p, 64, 1, 0, 1, p, None) == EINVAL
    assert b"frame_bytes" in L.fsea_last_error_string()
    assert L.fsea_trace_frames_host(fake, p, 64, 1, (1 << 31) + 1, 1, p) == EINVAL
    assert L.fsea_trace_frames_host(fake, p, 64, 1, 16, -1, p) == EINVAL                     # n_frames
    assert L.fsea_trace_frames_device(fake, p, 64, 1, 16, -1, p, None) == EINVAL
    assert L.fsea_trace_frames_host(fake, None, 64, 1, 16, 1, p) == EINVAL                   # bytes promised, none given
    assert L.fsea_trace_frames_device(fake, None, 64, 1, 16, 1, p, None) == EINVAL
    assert L.fsea_trace_frames_device(fake, p, 64, 1, 16, 1, p + 8, None) == EINVAL          # misaligned images
    assert L.fsea_trace_canvas_host(fake, None) == EINVAL
    assert not buf.any()


def test_trace_create_without_a_gpu_is_enodevice():
    L = fsea.hip_lib()
    t = ctypes.c_void_p()
    rc = L.fsea_trace_create(ctypes.byref(t), ctypes.byref(fsea.TraceConfig(1920, 1080, 4, 4, 0)), 0)
    if fsea.device_count() > 0:
        assert rc == 0 and t.value and L.fsea_trace_destroy(t) == 0
        return
    assert rc == ENODEVICE and not t.value
    with pytest.raises(fsea.FseaError):
        fsea.Trace()


def test_tool_is_built_and_rejects_bad_arguments(tmp_path):
    if not os.path.exists(TOOL):
        pytest.fail("fsea-single-sample is not built: run __graft_entry__.build()")
    cap = tmp_path / "capture.raw"
    np.zeros(400, np.uint8).tofile(str(cap))
    out = tmp_path / "out"
    out.mkdir()
    common = [TOOL, "--out", str(out)]
    for args in (["-p", "0"], ["-p", "255"], ["-f", "-1"], ["-f", "256"], ["-s", "0"], ["-s", "-4"], ["--multiplier", "0"],
                 ["--multiplier", "17"], ["--width", "1000"], ["--height", "100"], ["--bogus"], ["-p"]):
        r = subprocess.run(common + args + [str(cap)], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "fsea-single-sample" in r.stderr, args
        assert "fsea_trace_create" not in r.stderr, args          # refused before any device work
    r = subprocess.run(common, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no capture" in r.stderr
    r = subprocess.run(common + [str(cap), str(cap)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "usage" in r.stderr
    r = subprocess.run(common + [str(tmp_path / "nowhere.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cannot open capture" in r.stderr
    assert not list(out.iterdir())


def test_shipped_library_has_the_trace_kernels_without_spills():
    if not os.path.exists(LIB):
        pytest.fail("libfsea_hip.so is not built: run __graft_entry__.build()")
    ks = _kernels(LIB)
    names = sorted(k for k in ks if k.startswith("fsea_trace_"))
    assert names == ["fsea_trace_compose_b32", "fsea_trace_compose_b32_any", "fsea_trace_compose_b8",
                     "fsea_trace_compose_b8_any", "fsea_trace_hits_b32", "fsea_trace_hits_b8"]
    for name in names:
        k = ks[name]
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".group_segment_fixed_size"] == 0, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
    # the movie's kernel at the tool's geometry holds 16 canvas bytes and the counts of four frames (4 + 16 registers): with
    # at most 64 registers a SIMD holds its eight waves
    assert ks["fsea_trace_compose_b8"][".vgpr_count"] <= 64


@pytest.mark.skipif(not os.path.exists(os.path.join(generator().REF_C, "single-sample.c")), reason="reference tree absent")
def test_golden_generator_reproduces_the_committed_file(tmp_path, golden):
    import sys
    out = tmp_path / "trace_golden.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_trace_golden.py"), str(out)], check=True,
                   capture_output=True, timeout=600)
    with np.load(out) as z:
        again = {k: z[k] for k in z.files}
    assert sorted(again) == sorted(golden)
    for k in golden:
        assert np.array_equal(again[k], golden[k]), k
