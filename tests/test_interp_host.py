"""CPU tier of the interpolator and the gradual-noise movie: the numpy restatements (tests/interp_ref.py) against
tests/golden/interp_golden.npz (recorded from builds of the reference's own sources), the image tables of the C ABI against
the literal scatter loop, and the tool's weight sequence.  Nothing here needs a GPU."""
import hashlib
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import interp_ref as R
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "interp_golden.npz")
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-gradual-noise")


def generator():
    spec = importlib.util.spec_from_file_location("make_interp_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_interp_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_restated_interpolator_matches_the_reference(golden, kind):
    gen = generator()
    blocks, length, channels = gen.interp_inputs()[kind]
    for k, (step, calls) in enumerate(zip(gen.STEPS, gen.CALLS)):
        key = "%s__s%d" % (kind, k)
        ip = R.Interpolator(step)
        ts, recorded = [], list(golden["buf__%s__calls" % key])
        assert recorded == gen.RECORDED[k]
        for i in range(calls):
            ip.process(blocks[i % len(blocks)])
            ts.append(ip.t)
            if i in recorded:
                j = recorded.index(i)
                got = ip.get_buffer()
                assert np.array_equal(sha(got), golden["buf__%s__sha256" % key][j]), (key, i)
                assert float(got.astype(np.float64).sum()) == golden["buf__%s__sum" % key][j]
                whole = golden.get("buf__%s__c%d" % (key, i))
                if whole is not None:
                    assert got.dtype == whole.dtype and np.array_equal(got, whole)
        assert np.array_equal(np.array(ts), golden["t__" + key]), key          # bit for bit
    # what the issue states about the timing: swaps on calls 0, 101, 202 for 0.01, and t just above 1 before a swap
    t = golden["t__%s__s0" % kind]
    assert [i for i in range(1, 210) if t[i] == 0.0] == [101, 202]
    assert t[100] == 1.0000000000000007 and t[201] == 1.0000000000000007


def test_restated_movie_matches_the_reference_binary(golden):
    gen = generator()
    caps = gen.movie_captures()
    ts, eased, last = R.pair_weights(0.01)
    assert len(ts) == 100 and last == 1.0000000000000007
    sums_of = list(golden["movie__sums_of"])
    for pair in range(3):
        n = min(100, gen.MOVIE_FRAMES - 100 * pair)
        frames = R.image_frames(caps[pair], caps[pair + 1], eased[:n], gen.MOVIE_W, gen.MOVIE_H, 256)
        for k in range(n):
            no = 100 * pair + k + 1
            assert np.array_equal(sha(frames[k]), golden["movie__sha256"][no - 1]), no
            if no in sums_of:
                j = sums_of.index(no)
                assert np.array_equal(frames[k].astype(np.int64).sum(axis=1), golden["movie__rowsum"][j])
                assert np.array_equal(frames[k].astype(np.int64).sum(axis=0), golden["movie__colsum"][j])
            if no == gen.MOVIE_WHOLE:
                assert np.array_equal(frames[k], golden["movie__frame%d" % no])
    # the clamp's ends and the truncation are met: colours 0 and 255 occur, and some blend is no integer
    c = R.colours(caps[0], caps[1], eased[37], 256)
    assert c.min() == 0 and c.max() == 255


GEOMETRIES = [(1920, 1080, 256), (100, 60, 256), (48, 80, 32), (37, 23, 10), (5, 3, 8), (33, 33, 33), (16, 7, 3), (1, 1, 1),
              (250, 100, 100)]


@pytest.mark.parametrize("width,height,iq_size", GEOMETRIES)
def test_image_tables_equal_the_scatter_loop(width, height, iq_size):
    col, row = fsea.interp_image_tables(width, height, iq_size)
    ref_col, ref_row = R.scatter_tables(width, height, iq_size)
    assert np.array_equal(col, ref_col) and np.array_equal(row, ref_row)
    assert col.min() >= 0 and row.min() >= 0          # no pixel is left unwritten
    assert np.all(np.diff(col) >= 0) and np.all(np.diff(row) >= 0)
    if width * height * iq_size <= 48 * 80 * 32:
        # the tables say what the two nested loops of the tool leave in the image
        colours = (np.arange(iq_size * iq_size, dtype=np.int64) * 7 % 251 + 1).astype(np.uint8).reshape(iq_size, iq_size)
        assert np.array_equal(R.scatter_image(colours, width, height), colours[row][:, col])


def test_image_tables_of_the_tools_constants_have_the_closed_form():
    col, row = fsea.interp_image_tables(1920, 1080, 256)
    for tab in (col, row):
        p = np.arange(tab.size)
        assert np.array_equal(tab, 2 * (p // 15) + (p % 15 >= 7))
    assert row.max() == 143 and col.max() == 255


def test_image_tables_reject_bad_geometry():
    L = fsea.hip_lib()
    buf = np.zeros(16, dtype=np.int32)
    for w, h, s in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (16385, 4, 4), (4, 4, 4097), (-1, 4, 4)):
        assert L.fsea_interp_image_tables(w, h, s, buf.ctypes.data, buf.ctypes.data) == -1, (w, h, s)
    assert L.fsea_interp_image_tables(4, 4, 4, None, buf.ctypes.data) == -1


@pytest.mark.parametrize("step", [0.01, 0.3, 1.0, 0.07])
def test_tool_weight_sequence(step):
    if not os.path.exists(TOOL):
        pytest.fail("fsea-gradual-noise is not built: run __graft_entry__.build()")
    out = subprocess.run([TOOL, "--step", repr(step), "--print-weights"], capture_output=True, text=True, check=True).stdout
    got = [float.fromhex(x) for x in out.split()]
    ts, eased, _ = R.pair_weights(step)
    assert got == eased
    if step == 0.01:
        assert len(got) == 100


def test_tool_rejects_bad_arguments():
    for args in (["--step", "0"], ["--step", "-1"], ["--pattern", "rf-%s.raw"], ["--pattern", "rf.raw"], ["--bogus"]):
        r = subprocess.run([TOOL] + args + ["--print-weights"], capture_output=True, text=True)
        assert r.returncode != 0 and "fsea-gradual-noise" in r.stderr, args
