"""GPU tier: the persistence spectrum (fsea_persist_*, kernels fsea_persist_u8 / fsea_persist_f32 and their element-wise
forms, fsea_persist_image, fsea_persist_decay_u32), the nrf_persistence block and fsea-persistence.

Every comparison is bit for bit against tests/persist_ref.py applied to the very rows given to the object: the counts are
integers and do not depend on the order of the additions, so there is no tolerance anywhere.  The host form packs its rows at
a pitch of whole 16-byte groups (the 16-byte kernels from 16 bytes of row on); the device form with a pitch that is no
multiple of 16 bytes runs the element-wise kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import persist_ref as R
from tests.conftest import ROOT, synth_iq

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "frequensea_amd", "bin")
RUN = fsea.PERSIST_RUN_ROWS
MAPS = (fsea.PERSIST_MAP_SATURATE, fsea.PERSIST_MAP_LINEAR, fsea.PERSIST_MAP_LOG)


def device_counts(p, rows, pitch=None, lead=0):
    """The counts after a reset and one add_device of `rows` laid out `pitch` elements apart, `lead` elements (a multiple of
    16 bytes) behind the buffer's start."""
    n, width = rows.shape
    pitch = width if pitch is None else pitch
    flat = np.zeros(lead + max(n, 1) * pitch, rows.dtype)
    for r in range(n):
        flat[lead + r * pitch: lead + r * pitch + width] = rows[r]
    buf = fsea.DeviceBuffer(flat.nbytes).upload(flat)
    p.reset()
    p.add_device(buf.ptr.value + lead * rows.itemsize, fsea.PERSIST_U8 if rows.dtype == np.uint8 else fsea.PERSIST_F32, n, pitch)
    got = p.counts()
    buf.free()
    return got


@pytest.mark.parametrize("width", [1, 8, 50, 64, 100, 1000, 1024, 16384])
def test_random_u8_rows(width):
    """Row counts 0, 1, 3, 257 and one above a workgroup's run (16384 columns: 0, 1, 3, 70), host form and device form at
    pitch = width; then a pitch above the width in both kernels' forms, and a host array whose base is an odd column of
    wider rows."""
    rng = np.random.default_rng(width)
    n_max = 70 if width == 16384 else RUN + 1
    rows = rng.integers(0, 256, (n_max, width), dtype=np.uint8)
    rows[:, 0] = rng.integers(100, 104, n_max)                      # a column that piles up on four levels
    p = fsea.Persist(width)
    assert p.width == width and p.rows == 0 and not p.counts().any()
    for n in (0, 1, 3, 70) if width == 16384 else (0, 1, 3, 257, RUN + 1):
        want = R.counts_of(rows[:n])
        p.reset()
        p.add(rows[:n])
        assert p.rows == n and np.array_equal(p.counts(), want), (width, n, "host")
        assert np.array_equal(device_counts(p, rows[:n]), want), (width, n, "device")
        assert p.rows == n and want.sum() == n * width
    n = min(n_max, 300)
    want = R.counts_of(rows[:n])
    for pitch in (width + 5, (width + 15) // 16 * 16 + 16):
        assert np.array_equal(device_counts(p, rows[:n], pitch=pitch, lead=32), want), (width, pitch)
    wide = rng.integers(0, 256, (n, width + 9), dtype=np.uint8)
    off = 3 if wide.ctypes.data % 2 == 0 else 4
    band = wide[:, off:off + width]
    assert band.ctypes.data % 2 == 1 and band.strides == (width + 9, 1)
    p.reset()
    p.add(band)
    assert np.array_equal(p.counts(), R.counts_of(band)), (width, "sub-band of wider rows")
    p.close()


@pytest.mark.parametrize("form", ["host", "device"])
def test_contention_on_one_level(form):
    """70 000 rows of one constant byte at width 8: that level holds exactly 70 000 in every column (a 16-bit LDS counter
    would wrap, a lost same-address update would fall short); then the byte alternating between 0 and 255."""
    n, width = 70000, 8
    p = fsea.Persist(width)
    for rows in (np.full((n, width), 77, np.uint8), np.tile(np.array([[0], [255]], np.uint8), (n // 2, width))):
        if form == "host":
            p.reset()
            p.add(rows)
            got = p.counts()
        else:
            got = device_counts(p, rows)
        want = R.counts_of(rows)
        assert np.array_equal(got, want) and p.rows == n
        assert sorted(set(got.ravel().tolist())) in ([0, n], [0, n // 2])
    # the same through the 16-byte kernel: 64 columns, 16 rows of a wave on one level
    rows = np.full((n, 64), 200, np.uint8)
    p.close()
    p = fsea.Persist(64)
    got = device_counts(p, rows)
    assert (got[200] == n).all() and got.sum() == n * 64
    p.close()


def test_a_row_set_cut_into_three_calls_is_the_one_call_result():
    width, n = 100, 2 * RUN + 77
    rows = np.random.default_rng(1).integers(0, 256, (n, width), dtype=np.uint8)
    want = R.counts_of(rows)
    p = fsea.Persist(width)
    p.add(rows)
    assert np.array_equal(p.counts(), want) and p.rows == n
    p.reset()
    assert p.rows == 0 and not p.counts().any()
    done = 0
    for k in (1, RUN + 3, n - RUN - 4):
        p.add(rows[done:done + k])
        done += k
        assert p.rows == done
    assert done == n and np.array_equal(p.counts(), want)
    p.add(rows[:5])                                    # not reset: the counts go on
    assert p.rows == n + 5 and np.array_equal(p.counts(), R.counts_of(rows[:5], counts=want))
    p.close()


def f32_rows(width, n, lo, hi, seed):
    """Random values across [-120, 60], the exact boundaries lo + j / scale, lo, hi, nextafter(hi, -inf), both infinities
    and NaNs.  v - lo is 0 or at least an ulp of 70: |t| stays far from the denormal range."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-120, 60, (n, width)).astype(np.float32)
    scale = R.scale_of(lo, hi)
    special = np.concatenate([np.float32(lo) + np.arange(257, dtype=np.float32) / scale,
                              np.array([lo, hi, np.nextafter(np.float32(hi), np.float32(-np.inf)), np.inf, -np.inf, np.nan,
                                        np.nextafter(np.float32(lo), np.float32(-np.inf)), -0.0, 0.0], np.float32)])
    where = rng.choice(rows.size, size=min(rows.size // 2, 4 * special.size), replace=False)
    rows.ravel()[where] = special[np.arange(where.size) % special.size]
    return rows


@pytest.mark.parametrize("width", [1, 3, 50, 64, 200])
def test_f32_rows_with_a_range_whose_scale_is_no_power_of_two(width):
    lo, hi = -70.0, 30.0
    n = RUN + 19
    rows = f32_rows(width, n, lo, hi, width)
    want = R.counts_of(rows, lo, hi)
    nans = int(np.isnan(rows).sum())
    assert nans > 0 and np.isinf(rows).any() and R.scale_of(lo, hi) == np.float32(2.56)
    p = fsea.Persist(width)
    p.set_range(lo, hi)
    p.add(rows)
    got = p.counts()
    assert np.array_equal(got, want) and p.rows == n
    assert int(got.sum()) == n * width - nans                                    # a NaN is not counted
    assert np.array_equal(got.sum(axis=0), n - np.isnan(rows).sum(axis=0))
    assert np.array_equal(device_counts(p, rows), want)                           # pitch = width
    assert np.array_equal(device_counts(p, rows, pitch=width + 3, lead=4), want)
    assert np.array_equal(device_counts(p, rows, pitch=(width + 3) // 4 * 4 + 4, lead=8), want)
    p.reset()                                                                     # the range stays across a reset
    p.add(rows[:7])
    assert np.array_equal(p.counts(), R.counts_of(rows[:7], lo, hi))
    # the default range (-100, 0)
    q = fsea.Persist(width)
    q.add(rows)
    assert np.array_equal(q.counts(), R.counts_of(rows, -100.0, 0.0))
    p.close()
    q.close()


def staircase_rows(tiles):
    """300 rows of 8 columns (tiled): column k is at level 5 in its first c_k rows, c = 0, 1, 254, 255, 256, 300, 45, 299,
    and at level 200 + k in the others."""
    c = [0, 1, 254, 255, 256, 300, 45, 299]
    rows = np.empty((300, 8), np.uint8)
    for k in range(8):
        rows[:, k] = 200 + k
        rows[:c[k], k] = 5
    return np.tile(rows, (1, tiles))


@pytest.mark.parametrize("tiles", [1, 8, 25])
def test_the_three_maps_orientation_and_device_form(tiles):
    """Widths 8 and 200 (a pixel per lane) and 64 (16 pixels per lane); full 0 (= the 300 rows) and 100, below some counts."""
    rows = staircase_rows(tiles)
    width = rows.shape[1]
    counts = R.counts_of(rows)
    assert {0, 1, 254, 255, 256, 300} <= set(counts.ravel().tolist())
    p = fsea.Persist(width)
    for kind in MAPS:
        assert not p.image(kind).any() and not p.image(kind, full=9).any()      # nothing counted: a zero image
    p.add(rows)
    assert np.array_equal(p.counts(), counts)
    sync, st = fsea.Plan(64), fsea.Stream()
    d_image = fsea.DeviceBuffer(256 * width)
    for kind in MAPS:
        for full in (0, 100, 300, 1 << 40):
            want = R.image_of(counts, kind, full if full else 300)
            got = p.image(kind, full)
            assert np.array_equal(got, want), (kind, full)
            d_image.upload(np.full(256 * width, 0x5a, np.uint8))
            p.image_device(d_image.ptr.value, kind, full, stream=st)
            sync.synchronize(st)
            assert np.array_equal(d_image.download(np.uint8, (256, width)), want), (kind, full, "device")
    top = p.image(fsea.PERSIST_MAP_SATURATE)
    assert top[255 - 5, 1] == 1 and top[255 - 5, 3] == 255 and top[255 - 5, 4] == 255 and top[255 - 5, 0] == 0
    assert top[255 - 207, 7] == 1 and top[255 - 200, 0] == 255 and not top[:255 - 207].any()
    assert p.image(fsea.PERSIST_MAP_LOG)[255 - 5, 1] == 1                        # a single hit stays visible
    d_image.free()
    st.close()
    sync.close()
    p.close()


@pytest.mark.parametrize("width", [1, 50, 64])
def test_decay(width):
    rng = np.random.default_rng(width)
    rows = rng.integers(0, 7, (1500, width), dtype=np.uint8) * 36
    p = fsea.Persist(width)
    p.add(rows)
    counts, n = R.counts_of(rows), 1500
    for num, den in ((1, 2), (3, 4), (1, 1), (0xffffffff, 0xffffffff), (7, 9), (0, 1)):
        p.decay(num, den)
        counts, n = R.decay(counts, n, num, den)
        assert np.array_equal(p.counts(), counts) and p.rows == n, (num, den)
        assert np.array_equal(p.image(fsea.PERSIST_MAP_LINEAR), R.image_of(counts, R.MAP_LINEAR, n))
    assert n == 0 and not counts.any()
    p.add(rows[:9])                                                               # and it counts on afterwards
    assert p.rows == 9 and np.array_equal(p.counts(), R.counts_of(rows[:9]))
    p.close()


def test_device_form_on_callers_streams_equals_the_host_form():
    """One object fed from two streams in turn (its event orders them), and two objects on two streams."""
    width, n = 1024, 600
    rows = np.random.default_rng(2).integers(0, 256, (n, width), dtype=np.uint8)
    host = fsea.Persist(width)
    host.add(rows)
    want = host.counts()
    assert np.array_equal(want, R.counts_of(rows))
    s1, s2 = fsea.Stream(), fsea.Stream()
    d_rows = fsea.DeviceBuffer(rows.nbytes).upload(rows)
    a, b = fsea.Persist(width), fsea.Persist(width)
    half = 304 * width
    a.add_device(d_rows.ptr.value, fsea.PERSIST_U8, 304, width, stream=s1)
    b.add_device(d_rows.ptr.value, fsea.PERSIST_U8, n, width, stream=s2)
    a.add_device(d_rows.ptr.value + half, fsea.PERSIST_U8, n - 304, width, stream=s2)
    a.decay(1, 1, stream=s1)
    assert np.array_equal(a.counts(), want) and np.array_equal(b.counts(), want) and a.rows == b.rows == n
    for k in range(4):                                                            # alternate streams, no wait in between
        a.add_device(d_rows.ptr.value, fsea.PERSIST_U8, 100, width, stream=(s1, s2)[k % 2])
    assert np.array_equal(a.counts(), R.counts_of(np.tile(rows[:100], (4, 1)), counts=want))
    d_rows.free()
    for o in (a, b, host):
        o.close()
    s1.close()
    s2.close()


def check_teeth(counts, what):
    levels = int((counts.sum(axis=1) > 0).sum())
    print("%s: %d levels occupied" % (what, levels))
    assert levels >= 64 and (counts.sum(axis=0) > 0).all(), (what, levels)


@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("mode", [fsea.MODE_DB5_U8_DCFIX, fsea.MODE_DB10_U8])
def test_a_plans_resident_rows(golden_all, N, mode):
    """The golden block through a plan on the device, its rows fed to the object without leaving it; the restatement on the
    plan's own fetched rows."""
    block = np.ascontiguousarray(golden_all["block__raw"])
    frames = block.size // 2 // N
    plan = fsea.Plan(N, N, mode)
    d_iq = fsea.DeviceBuffer(block.nbytes).upload(block)
    d_rows = fsea.DeviceBuffer(frames * N)
    plan.exec_device(d_iq.ptr.value, frames, d_rows.ptr.value, flip=True)
    p = fsea.Persist(N)
    p.add_device(d_rows.ptr.value, fsea.PERSIST_U8, frames, N)
    got = p.counts()
    rows = d_rows.download(np.uint8, (frames, N))
    want = R.counts_of(rows)
    check_teeth(want, "N %d mode %d" % (N, mode))
    assert np.array_equal(got, want) and p.rows == frames
    # a sub-band of the rows: columns N/4 .. 3N/4 at the wide pitch
    q = fsea.Persist(N // 2)
    q.add_device(d_rows.ptr.value + N // 4, fsea.PERSIST_U8, frames, N)
    assert np.array_equal(q.counts(), want[:, N // 4: 3 * N // 4])
    for o in (p, q, plan):
        o.close()
    d_iq.free()
    d_rows.free()


def test_a_db_f32_plans_resident_rows_with_a_range(golden_all):
    N = 1024
    block = np.ascontiguousarray(golden_all["block__raw"])
    frames = block.size // 2 // N
    plan = fsea.Plan(N, N, fsea.MODE_DB_F32)
    d_iq = fsea.DeviceBuffer(block.nbytes).upload(block)
    d_rows = fsea.DeviceBuffer(frames * N * 4)
    plan.exec_device(d_iq.ptr.value, frames, d_rows.ptr.value, flip=True)
    p = fsea.Persist(N)
    p.set_range(0.0, 40.0)
    p.add_device(d_rows.ptr.value, fsea.PERSIST_F32, frames, N)
    got = p.counts()
    rows = d_rows.download(np.float32, (frames, N))
    want = R.counts_of(rows, 0.0, 40.0)
    check_teeth(want, "DB_F32")
    assert np.array_equal(got, want) and p.rows == frames
    p.close()
    plan.close()
    d_iq.free()
    d_rows.free()


def test_a_zooms_and_a_banks_resident_rows(golden_all):
    block = np.ascontiguousarray(golden_all["block__raw"])
    n = block.size // 2
    d_iq = fsea.DeviceBuffer(block.nbytes).upload(block)
    zoom = fsea.Zoom(fsea.lowpass_taps(8000000, 900000, 64), 4, 256, 256, fsea.MODE_DB10_U8)
    bank = fsea.Pfb(fsea.pfb_prototype(128, 8), 128, 2, fsea.MODE_DB10_U8)
    for what, obj, width, n_rows, run in (
            ("zoom", zoom, 256, zoom.out_rows(n), lambda d: zoom.run_device(d_iq.ptr.value, n, d, 0.05, flip=True)),
            ("pfb", bank, 128, bank.out_frames(n), lambda d: bank.run_device(d_iq.ptr.value, n, d, flip=True))):
        d_rows = fsea.DeviceBuffer(n_rows * width)
        run(d_rows.ptr.value)
        p = fsea.Persist(width)
        p.add_device(d_rows.ptr.value, fsea.PERSIST_U8, n_rows, width)
        got = p.counts()
        want = R.counts_of(d_rows.download(np.uint8, (n_rows, width)))
        check_teeth(want, what)
        assert np.array_equal(got, want) and p.rows == n_rows, what
        p.close()
        d_rows.free()
        obj.close()
    d_iq.free()


def _picture(L, p, N):
    buf = L.nrf_persistence_get_buffer(p)
    c = buf.contents
    assert (c.type, c.length, c.channels, c.size_bytes) == (nrf.NUT_BUFFER_U8, 256 * N, 1, 256 * N)
    img = nrf.buffer_to_numpy(L, buf).reshape(256, N).copy()
    L.nut_buffer_free(buf)                             # the caller's to free
    return img


@pytest.mark.parametrize("decay", [None, (3, 4)])
def test_host_block_counts_the_plans_rows(golden_all, decay):
    L = nrf.nrf_lib()
    N, hop = 128, 64
    block = np.ascontiguousarray(golden_all["block__raw"] ^ 0x80)
    n = block.size // 2
    frames = (n - N) // hop + 1
    plan = fsea.Plan(N, hop, fsea.MODE_DB5_U8_DCFIX)
    plan.set_window("hann")
    rows = plan.exec_host(block, frames, flip=False)
    plan.close()
    assert rows.shape == (frames, N)
    p = L.nrf_persistence_new(N, hop, fsea.PERSIST_MAP_LOG)
    L.nrf_persistence_set_window(p, b"hann")
    if decay:
        L.nrf_persistence_set_decay(p, *decay)
    assert not _picture(L, p, N).any()
    counts, total = np.zeros((256, N), np.uint32), 0
    for k in range(2):
        buf = L.nut_buffer_new_u8(n, 2, block.ctypes.data)
        L.nrf_persistence_process(p, buf)
        L.nut_buffer_free(buf)
        if decay:
            counts, total = R.decay(counts, total, *decay)
        counts, total = R.counts_of(rows, counts=counts), total + frames
        assert np.array_equal(_picture(L, p, N), R.image_of(counts, R.MAP_LOG, total)), (decay, k)
    short = L.nut_buffer_new_u8(N - 1, 2, block.ctypes.data)       # shorter than a frame: nothing is added
    L.nrf_persistence_process(p, short)
    L.nut_buffer_free(short)
    if decay:
        counts, total = R.decay(counts, total, *decay)
    assert np.array_equal(_picture(L, p, N), R.image_of(counts, R.MAP_LOG, total))
    L.nrf_persistence_free(p)


def test_host_block_refuses_an_f64_buffer():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n"
            "p = L.nrf_persistence_new(128, 128, 2)\n"
            "L.nrf_persistence_process(p, L.nut_buffer_new_f64(4096, 2, None))\n"
            "print('returned')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF PERSISTENCE fatal error" in r.stderr and "F64" in r.stderr


def test_tool_writes_the_picture_and_the_traces(tmp_path):
    from PIL import Image
    N, hop, n_frames = 256, 128, 599
    raw = synth_iq(7, 2 * ((n_frames - 1) * hop + N) + 2 * 50)                 # 50 samples over: no further frame
    raw.tofile(tmp_path / "tone.raw")
    out, traces = tmp_path / "p.png", tmp_path / "traces.txt"
    r = subprocess.run([os.path.join(BIN, "fsea-persistence"), str(tmp_path / "tone.raw"), "--size", str(N), "--hop", str(hop),
                        "--window", "hann", "--flip", "--map", "log", "--traces", str(traces), "-o", str(out)],
                       capture_output=True, text=True, check=True, timeout=300)
    plan = fsea.Plan(N, hop, fsea.MODE_DB5_U8_DCFIX)
    plan.set_window("hann")
    rows = plan.exec_host(raw, n_frames, flip=True)
    plan.close()
    counts = R.counts_of(rows)
    with Image.open(out) as im:
        got = np.array(im)
    assert got.dtype == np.uint8 and np.array_equal(got, R.image_of(counts, R.MAP_LOG, n_frames))
    want = [fsea.persist_trace(counts, kind, 0.5) for kind in (fsea.PERSIST_TRACE_MAX, fsea.PERSIST_TRACE_QUANTILE,
                                                               fsea.PERSIST_TRACE_MIN)]
    table = np.loadtxt(traces, dtype=np.int64)
    assert table.shape == (N, 4) and np.array_equal(table[:, 0], np.arange(N))
    for j in range(3):
        assert np.array_equal(table[:, 1 + j], want[j]) and np.array_equal(want[j], R.trace(counts, (0, 2, 1)[j], 0.5))
    # the tone at + rate / 8; the offset-binary DC term under the Hann window fills columns N/2 - 1 .. N/2 + 1 and is left out
    away = want[0].astype(int)
    away[N // 2 - 2: N // 2 + 3] = 0
    assert int(np.argmax(away)) == N // 2 + N // 8 and want[0][N // 2 + N // 8] > want[1][N // 2 + N // 8 + 10] + 50
    assert "rows %d" % n_frames in r.stdout
    assert "levels %d to %d" % (want[2].min(), want[0].max()) in r.stdout
    # f32 dB rows over a range, the LINEAR map with an explicit full scale
    r = subprocess.run([os.path.join(BIN, "fsea-persistence"), str(tmp_path / "tone.raw"), "--size", str(N), "--flip", "--mode",
                        "db:-10:40", "--map", "lin", "--full", "50", "-o", str(out)], capture_output=True, text=True,
                       check=True, timeout=300)
    plan = fsea.Plan(N, N, fsea.MODE_DB_F32)
    rows = plan.exec_host(raw, raw.size // 2 // N, flip=True)
    plan.close()
    with Image.open(out) as im:
        got = np.array(im)
    assert np.array_equal(got, R.image_of(R.counts_of(rows, -10.0, 40.0), R.MAP_LINEAR, 50))
