"""GPU tier: the CFAR spectrum detector (fsea_cfar_*, kernels fsea_cfar_u8 / fsea_cfar_f32 and their element-wise forms),
the nrf_spectrum_occupancy block and fsea-occupancy.

Every comparison is bit for bit against tests/cfar_ref.py applied to the very rows given to the object: mask, row hits,
hits and rows are integers and do not depend on the order of the additions, so there is no tolerance anywhere.  The device
form's outputs are tests/guarded.py payloads of exactly the documented size: a store outside them
dirties a band.  The host form packs its rows at a pitch of whole 16-byte groups (the 16-byte kernels); the device form with
a pitch that is no multiple of 16 bytes runs the element-wise kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import cfar_ref as R
from tests.conftest import ROOT, synth_iq
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "frequensea_amd", "bin")
TILE, RUN = fsea.CFAR_TILE_COLUMNS, fsea.CFAR_RUN_ROWS
DEFAULT = (2, 16, 60, R.CA)
GARBAGE = 0xDEADBEEF


def device_run(c, rows, pitch=None, lead=0, fence=0x00, mask=True, row_hits=True, stream=0, reset=True):
    """One add_device of `rows` laid out `pitch` elements apart, `lead` elements (a multiple of 16 bytes) behind the start of
    a buffer otherwise full of `fence` bytes; mask and row hits into guarded payloads of exactly n * width bytes and n
    uint32 (pre-filled, the row hits with garbage).  Returns (mask, row_hits, hits, rows); None for what was not asked."""
    n, width = rows.shape
    pitch = width if pitch is None else pitch
    flat = np.full((lead + max(n, 1) * pitch) * rows.itemsize, fence, np.uint8).view(rows.dtype).copy()
    for r in range(n):
        flat[lead + r * pitch: lead + r * pitch + width] = rows[r]
    g_in = Guarded(flat.nbytes, fill=fence).upload(flat)
    g_mask = Guarded(n * width) if mask else None
    g_hits = Guarded(4 * n) if row_hits else None
    if row_hits and n:
        g_hits.upload(np.full(n, GARBAGE, np.uint32))
    if reset:
        c.reset()
    c.add_device(g_in.addr + lead * rows.itemsize, fsea.CFAR_U8 if rows.dtype == np.uint8 else fsea.CFAR_F32, n, pitch,
                 g_mask.addr if mask else None, g_hits.addr if row_hits else None, stream=stream)
    hits = c.hits()                                            # behind the add, whatever its stream
    got_mask = g_mask.payload(np.uint8, (n, width)) if mask else None
    got_hits = g_hits.payload(np.uint32, (n,)) if row_hits else None
    for g, what in ((g_mask, "mask"), (g_hits, "row hits"), (g_in, "input")):
        if g is not None:
            g.check(what)
            g.free()
    return got_mask, got_hits, hits, c.rows


def check(c, rows, settings=DEFAULT, what="", **kw):
    """Device form (guarded) and host form against the restatement; returns the expected mask."""
    c.set(*settings)
    want = R.detect(rows, *settings)
    m, h, hits, n = device_run(c, rows, **kw)
    assert np.array_equal(m, want), (what, "mask", int((m != want).sum()), np.argwhere(m != want)[:4].tolist())
    assert np.array_equal(h, R.row_hits_of(want)), (what, "row hits")
    assert np.array_equal(hits, R.hits_of(want)) and n == rows.shape[0], (what, "hits")
    c.reset()
    hm, hh = c.add(rows, mask=True, row_hits=True)
    assert np.array_equal(hm, want) and np.array_equal(hh, R.row_hits_of(want)), (what, "host form")
    assert np.array_equal(c.hits(), R.hits_of(want)) and c.rows == rows.shape[0], (what, "host form hits")
    return want


@pytest.mark.parametrize("width", [1, 2, 15, 16, 17, 1000, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_random_u8_rows(width):
    """Full-range random bytes; 1, RUN - 1 and RUN + 1 rows; pitch = width and width + 5 (the element-wise kernel) and, at a
    multiple of 16 above the width, the 16-byte kernel on rows whose last group is partial."""
    rng = np.random.default_rng(width)
    rows = rng.integers(0, 256, (RUN + 1, width), dtype=np.uint8)
    c = fsea.Cfar(width)
    assert c.width == width and c.rows == 0 and not c.hits().any()
    for n in (1, RUN - 1, RUN + 1):
        want = check(c, rows[:n], what=(width, n))
        assert width < 8 or want.any()
    for pitch in (width + 5, (width + 15) // 16 * 16 + 16):
        check(c, rows[:RUN + 1], pitch=pitch, lead=32, fence=0xFF, what=(width, "pitch", pitch))
    c.close()


@pytest.mark.parametrize("width,settings", [(200, (64, 256, 10, R.CA)), (300, (64, 256, 0, R.GO)), (TILE + 700, (64, 256, 20, R.CA)),
                                            (TILE + 700, (64, 256, 20, R.SO)), (2 * TILE, (64, 256, 30, R.GO))])
def test_the_widest_windows(width, settings):
    """A width below G + T, where every window is clipped, and widths whose windows reach across a tile seam."""
    rows = np.random.default_rng(width).integers(0, 256, (5, width), dtype=np.uint8)
    c = fsea.Cfar(width)
    want = check(c, rows, settings, what=(width, settings))
    assert want.any()
    check(c, rows, settings, pitch=width + 5, what=(width, settings, "element-wise"))
    c.close()


def test_a_sub_band_of_wider_rows():
    """Columns 48 .. 48 + width of rows 1500 wide, on the device at the wide pitch (16-byte kernel: 1500 is no multiple of
    16, so element-wise; 1504 is) and from a host array with an odd base."""
    rng = np.random.default_rng(5)
    for wide_w, width in ((1504, 1100), (1500, 1100), (1504, 7)):
        wide = rng.integers(0, 256, (9, wide_w), dtype=np.uint8)
        band = wide[:, 48:48 + width]
        want = R.detect(band, *DEFAULT)
        buf = fsea.DeviceBuffer(wide.nbytes).upload(wide)
        g_mask = Guarded(band.size)
        c = fsea.Cfar(width)
        c.add_device(buf.ptr.value + 48, fsea.CFAR_U8, 9, wide_w, g_mask.addr)
        assert np.array_equal(c.hits(), R.hits_of(want)), (wide_w, width)
        assert np.array_equal(g_mask.payload(np.uint8, band.shape), want)
        g_mask.check("mask of a sub-band")
        odd = wide[:, 3:3 + width] if wide.ctypes.data % 2 == 0 else wide[:, 4:4 + width]
        c.reset()
        assert np.array_equal(c.add(odd, mask=True), R.detect(odd, *DEFAULT))
        c.close()
        g_mask.free()
        buf.free()


@pytest.mark.parametrize("settings", [(0, 16, 60, R.CA), (2, 1, 60, R.CA), (0, 1, 0, R.SO), (64, 256, 60, R.CA), (2, 16, -3, R.CA),
                                      (2, 16, 0, R.GO), (2, 16, 255, R.CA), (2, 16, 255, R.SO), (3, 7, -3, R.GO)])
def test_settings(settings):
    width = TILE + 37
    rows = np.random.default_rng(11).integers(0, 256, (6, width), dtype=np.uint8)
    c = fsea.Cfar(width)
    want = check(c, rows, settings, what=settings)
    if settings[2] == 255:
        assert not want.any()                                  # a u8 level cannot stand 255 above a mean of u8 levels
    else:
        assert want.any()
    c.close()


def test_the_three_methods_differ_on_a_step():
    """Level 40 left of column 600 and 120 from it on, plus noise of +-3 and two carriers beside the step: CA fires along
    the upper edge of the step, GO does not, SO fires on more; the three masks differ from one another."""
    rng = np.random.default_rng(3)
    width = 1200
    rows = np.where(np.arange(width) < 600, 40, 120)[None, :] + rng.integers(-3, 4, (8, width))
    rows[:, 300] += 80
    rows[:, 606] += 50
    rows = rows.astype(np.uint8)
    c = fsea.Cfar(width)
    masks = [check(c, rows, (2, 16, 30, m), what=("step", m)) for m in (R.CA, R.GO, R.SO)]
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[0], masks[2]) and not np.array_equal(masks[1], masks[2])
    assert masks[0][:, 600:603].all() and not masks[1][:, 600:606].any() and masks[1][:, 300].all()
    assert (masks[2] >= masks[0]).all() and (masks[0] >= masks[1]).all()
    c.close()


@pytest.mark.parametrize("value", [0, 255])
def test_constant_rows(value):
    width = TILE + 16
    rows = np.full((3, width), value, np.uint8)
    c = fsea.Cfar(width)
    assert not check(c, rows, (2, 16, 0, R.CA), what=value).any()            # x * n > S is strict
    assert check(c, rows, (2, 16, -1, R.GO), what=value).all()
    c.close()


def f32_special_rows(width, n, seed):
    """dB values in [-120, 20], every clamp and NaN, and values whose 64-fold is exactly halfway between two integers."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-120, 20, (n, width)).astype(np.float32)
    half = (np.arange(-40, 40, dtype=np.float32) + np.float32(0.5)) / np.float32(64)
    special = np.concatenate([half, np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 16384.0, -16384.0, 16383.99, -16383.99, 0.0,
                                              -0.0, 3e38, -3e38], np.float32)])
    where = rng.choice(rows.size, size=min(rows.size // 3, 3 * special.size), replace=False)
    rows.ravel()[where] = special[np.arange(where.size) % special.size]
    return rows


@pytest.mark.parametrize("width", [1, 3, 4, 50, 1000, TILE + 5])
def test_f32_rows(width):
    rows = f32_special_rows(width, RUN + 1, width)
    lv = R.levels_of_f32(rows)
    assert width < 50 or ({-R.LIMIT, R.LIMIT} <= set(lv.ravel().tolist()) and np.isnan(rows).any())
    assert R.levels_of_f32(np.array([0.5 / 64, 1.5 / 64, 2.5 / 64, -0.5 / 64, -1.5 / 64], np.float32)).tolist() == [0, 2, 2, 0, -2]
    c = fsea.Cfar(width)
    for settings in ((2, 16, 60 * 64, R.CA), (1, 5, 0, R.GO), (0, 3, -(1 << 20), R.SO), (64, 256, 1 << 20, R.CA)):
        check(c, rows, settings, what=(width, settings))
    check(c, rows[:5], (2, 16, 640, R.SO), pitch=width + 3, lead=4, fence=0xFF, what=(width, "element-wise"))   # 0xFF: NaNs
    check(c, rows[:5], (2, 16, 640, R.CA), pitch=(width + 3) // 4 * 4 + 4, lead=8, what=(width, "partial group"))
    c.close()


def test_f32_prefix_sums_that_wrap():
    """6000 cells at the upper clamp: their sum passes 2^32 (and the lower clamp's passes -2^32); a cell is a hit exactly
    where the restatement's 64-bit sums say so."""
    width = 6000
    rows = np.full((3, width), 1e9, np.float32)
    rows[1] = -1e9
    rows[2, ::7] = -1e9
    rows[0, 4500] = np.nan
    rows[1, 4500] = 5.0
    assert abs(int(R.levels_of_f32(rows[0]).sum())) > 1 << 32 and abs(int(R.levels_of_f32(rows[1]).sum())) > 1 << 32
    c = fsea.Cfar(width)
    for settings in ((2, 16, 0, R.CA), (64, 256, -1, R.GO), (0, 256, 1 << 20, R.SO), (0, 200, -(1 << 20), R.CA)):
        check(c, rows, settings, what=("wrap", settings))
    want = R.detect(rows, 2, 16, 0, R.CA)
    assert want[1, 4500] == 255 and want[0].any() and want[2].any() and not want.all()
    c.close()


def test_cut_invariance_and_two_streams():
    """The same rows in one call, in calls of 1 and of 3 rows, and in halves on two streams: the same hits and rows."""
    width, n = TILE + 100, 13
    rows = np.random.default_rng(8).integers(0, 256, (n, width), dtype=np.uint8)
    want = R.detect(rows, *DEFAULT)
    c = fsea.Cfar(width)
    c.add(rows)
    assert np.array_equal(c.hits(), R.hits_of(want)) and c.rows == n
    c.reset()
    c.add(rows[:1])
    for r in range(1, n, 3):
        c.add(rows[r:r + 3])
    assert np.array_equal(c.hits(), R.hits_of(want)) and c.rows == n
    c.reset()
    s1, s2 = fsea.Stream(), fsea.Stream()
    d_rows = fsea.DeviceBuffer(rows.nbytes).upload(rows)
    d_mask = fsea.DeviceBuffer(rows.nbytes)
    assert (8 * width) % 16 == 0                                                          # the second part's base is aligned
    c.add_device(d_rows.ptr.value, fsea.CFAR_U8, 8, width, d_mask.ptr.value, stream=s1)
    c.add_device(d_rows.ptr.value + 8 * width, fsea.CFAR_U8, n - 8, width, d_mask.ptr.value + 8 * width, stream=s2)
    c.add_device(d_rows.ptr.value, fsea.CFAR_U8, n, width, stream=s1)                      # no wait in between
    assert np.array_equal(c.hits(), 2 * R.hits_of(want)) and c.rows == 2 * n
    assert np.array_equal(d_mask.download(np.uint8, rows.shape), want)
    for o in (d_rows, d_mask):
        o.free()
    for o in (s1, s2, c):
        o.close()


def test_optional_outputs_and_reset():
    width, n = 333, 7
    rows = np.random.default_rng(9).integers(0, 256, (n, width), dtype=np.uint8)
    settings = (1, 9, 40, R.GO)
    want = R.detect(rows, *settings)
    c = fsea.Cfar(width)
    c.set(*settings)
    m, h, hits, _ = device_run(c, rows, mask=True, row_hits=False)
    assert h is None and np.array_equal(m, want) and np.array_equal(hits, R.hits_of(want))
    m, h, hits, _ = device_run(c, rows, mask=False, row_hits=True)
    assert m is None and np.array_equal(h, R.row_hits_of(want)) and np.array_equal(hits, R.hits_of(want))
    m, h, hits, total = device_run(c, rows, mask=False, row_hits=False, reset=False)
    assert m is None and h is None and np.array_equal(hits, 2 * R.hits_of(want)) and total == 2 * n
    assert c.add(rows) is None and c.rows == 3 * n
    assert np.array_equal(c.add(rows, row_hits=True), R.row_hits_of(want))
    c.add(rows[:0])                                                               # no rows: a successful no-op
    c.add_device(0, fsea.CFAR_U8, 0, width)
    assert c.rows == 4 * n
    c.reset()                                                                     # zeroes hits and rows, keeps the settings
    assert c.rows == 0 and not c.hits().any()
    assert np.array_equal(c.add(rows, mask=True), want)
    c.close()
    for _ in range(20):                                                           # create / destroy cycles
        c = fsea.Cfar(64)
        c.add(rows[:2, :64])
        c.close()


def test_the_input_fence_does_not_move_the_result():
    """Rows fenced with bands of 0x00 and of 0xFF, in front, behind and in the gap between the rows' ends and the pitch: the
    same mask, so nothing outside a row's width is read into a result."""
    width = TILE - 3
    rows = np.random.default_rng(12).integers(0, 256, (4, width), dtype=np.uint8)
    c = fsea.Cfar(width)
    c.set(64, 256, 10, R.CA)
    want = R.detect(rows, 64, 256, 10, R.CA)
    for pitch in (width, width + 3, width + 19):
        for fence in (0x00, 0xFF):
            m, h, hits, _ = device_run(c, rows, pitch=pitch, lead=16, fence=fence)
            assert np.array_equal(m, want) and np.array_equal(h, R.row_hits_of(want)), (pitch, fence)
    c.close()


@pytest.mark.parametrize("N,frames", [(256, 64), (1024, 32)])
def test_a_plans_resident_rows(N, frames):
    """synth_iq(7) through a DB5 plan on the device into the object; no row visits the host in between.  The tone's column is
    hit in every row under CA and GO, and outside tone +- 2 and DC +- 2 at most 0.2 % of the cells are (a numpy restatement
    of these rows gave 0 of 15 744 cells at N = 256 and 9 (CA) and 4 (GO) of 32 448 at N = 1024)."""
    raw = synth_iq(7, 2 * N * frames)
    plan = fsea.Plan(N, N, fsea.MODE_DB5_U8_DCFIX)
    d_iq = fsea.DeviceBuffer(raw.nbytes).upload(raw)
    d_rows = fsea.DeviceBuffer(frames * N)
    plan.exec_device(d_iq.ptr.value, frames, d_rows.ptr.value, flip=True)
    rows = d_rows.download(np.uint8, (frames, N))
    tone, dc = N // 2 + N // 8, N // 2
    away = np.ones(N, bool)
    away[tone - 2: tone + 3] = False
    away[dc - 2: dc + 3] = False
    c = fsea.Cfar(N)
    for method in (R.CA, R.GO, R.SO):
        c.set(2, 16, 60, method)
        c.reset()
        g_mask = Guarded(frames * N)
        c.add_device(d_rows.ptr.value, fsea.CFAR_U8, frames, N, g_mask.addr)
        want = R.detect(rows, 2, 16, 60, method)
        hits = c.hits()
        assert np.array_equal(g_mask.payload(np.uint8, (frames, N)), want) and np.array_equal(hits, R.hits_of(want)), method
        g_mask.check("mask")
        g_mask.free()
        false_alarms, cells = int(hits[away].sum()), frames * int(away.sum())
        print("N %d method %d: tone column %d of %d rows, %d of %d cells away from tone and DC" % (N, method, hits[tone], frames,
                                                                                                   false_alarms, cells))
        if method != R.SO:
            assert hits[tone] == frames and false_alarms <= 0.002 * cells, (method, hits[tone], false_alarms)
            bands = fsea.cfar_bands(hits, frames, 0.9, max_gap=1)
            assert tone in [int(b["peak"]) for b in bands]
    for o in (c, plan):
        o.close()
    d_iq.free()
    d_rows.free()


def test_a_db_f32_plans_resident_rows(golden_all):
    N = 1024
    block = np.ascontiguousarray(golden_all["block__raw"])
    frames = 40
    plan = fsea.Plan(N, N, fsea.MODE_DB_F32)
    d_iq = fsea.DeviceBuffer(block.nbytes).upload(block)
    d_rows = fsea.DeviceBuffer(frames * N * 4)
    plan.exec_device(d_iq.ptr.value, frames, d_rows.ptr.value, flip=True)
    rows = d_rows.download(np.float32, (frames, N))
    c = fsea.Cfar(N)
    c.set(2, 16, 6 * 64, R.CA)                                                    # 6 dB above the neighbours' mean level
    g_mask = Guarded(frames * N)
    c.add_device(d_rows.ptr.value, fsea.CFAR_F32, frames, N, g_mask.addr)
    want = R.detect(rows, 2, 16, 6 * 64, R.CA)
    assert want.any() and not want.all()
    assert np.array_equal(g_mask.payload(np.uint8, (frames, N)), want) and np.array_equal(c.hits(), R.hits_of(want))
    g_mask.check("mask")
    g_mask.free()
    c.close()
    plan.close()
    d_iq.free()
    d_rows.free()


def _recording(tmp_path, N, hop, n_frames):
    raw = synth_iq(7, 2 * ((n_frames - 1) * hop + N) + 2 * 50)                 # 50 samples over: no further frame
    raw.tofile(tmp_path / "tone.raw")
    plan = fsea.Plan(N, hop, fsea.MODE_DB5_U8_DCFIX)
    plan.set_window("hann")
    rows = plan.exec_host(raw, n_frames, flip=True)
    plan.close()
    return raw, rows


def _bands_file(path):
    text = open(path).read().split("\n")
    return [tuple(line.split()) for line in text if line]


def test_tool_writes_the_mask_and_the_bands(tmp_path):
    from PIL import Image
    N, hop, n_frames = 256, 128, 99
    raw, rows = _recording(tmp_path, N, hop, n_frames)
    out, bands_path = tmp_path / "mask.png", tmp_path / "bands.txt"
    tool = os.path.join(BIN, "fsea-occupancy")
    r = subprocess.run([tool, str(tmp_path / "tone.raw"), "--size", str(N), "--hop", str(hop), "--window", "hann", "--flip",
                        "--guard", "3", "--train", "12", "--offset", "50", "--method", "go", "--min-duty", "0.5", "--max-gap", "1",
                        "--rate", "8000000", "--freq", "100", "--mask", str(out), "--bands", str(bands_path)],
                       capture_output=True, text=True, check=True, timeout=300)
    want = R.detect(rows, 3, 12, 50, R.GO)
    with Image.open(out) as im:
        got = np.array(im)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    bands = R.bands_of(R.hits_of(want), n_frames, 0.5, 1, 1)
    tone = N // 2 + N // 8
    assert any(b["first"] <= tone <= b["last"] for b in bands)     # under the Hann window the tone fills three columns

    def mhz(k):
        return "%.6f" % (100.0 + (k - N // 2) * 8000000.0 / N / 1e6)

    lines = ["%d %d %d %.6f %s %s %s" % (b["first"], b["last"], b["peak"], b["peak_hits"] / n_frames, mhz(b["first"]), mhz(b["last"]),
                                         mhz(b["peak"])) for b in bands]
    assert r.stdout.split("\n")[0] == "rows %d" % n_frames and r.stdout.split("\n")[1:1 + len(lines)] == lines
    assert _bands_file(bands_path) == [tuple(line.split()) for line in lines]
    assert mhz(tone) == "101.000000"                                             # + rate / 8 above the centre
    # the same rows as an 8-bit grey image: the same bands, without the MHz columns
    Image.fromarray(rows).save(tmp_path / "rows.png")
    r2 = subprocess.run([tool, "--image", str(tmp_path / "rows.png"), "--guard", "3", "--train", "12", "--offset", "50", "--method",
                         "go", "--min-duty", "0.5", "--max-gap", "1", "--mask", str(out)], capture_output=True, text=True,
                        check=True, timeout=300)
    assert r2.stdout.split("\n")[0] == "rows %d" % n_frames
    assert r2.stdout.split("\n")[1:1 + len(lines)] == [" ".join(line.split()[:4]) for line in lines]
    with Image.open(out) as im:
        assert np.array_equal(np.array(im), want)


def test_host_block_duty_and_mask_are_the_objects(tmp_path):
    L = nrf.nrf_lib()
    N, hop, n_frames = 128, 64, 77
    raw, rows = _recording(tmp_path, N, hop, n_frames)
    block = np.ascontiguousarray(raw ^ 0x80)                                     # offset binary, as the device's buffers are
    p = L.nrf_spectrum_occupancy_new(N, hop, 1, 9, 45, fsea.CFAR_SO)
    L.nrf_spectrum_occupancy_set_window(p, b"hann")

    def duty():
        buf = L.nrf_spectrum_occupancy_get_buffer(p)
        k = buf.contents
        assert (k.type, k.length, k.channels) == (nrf.NUT_BUFFER_F64, N, 1)
        out = nrf.buffer_to_numpy(L, buf).copy()
        L.nut_buffer_free(buf)
        return out

    def mask():
        buf = L.nrf_spectrum_occupancy_get_mask_buffer(p)
        k = buf.contents
        assert k.type == nrf.NUT_BUFFER_U8 and k.channels == 1
        out = nrf.buffer_to_numpy(L, buf).copy() if k.length else np.zeros(0, np.uint8)
        L.nut_buffer_free(buf)
        return out

    assert not duty().any() and mask().size == 0
    c = fsea.Cfar(N)
    c.set(1, 9, 45, fsea.CFAR_SO)
    for k in range(2):
        buf = L.nut_buffer_new_u8(raw.size // 2, 2, block.ctypes.data)
        L.nrf_spectrum_occupancy_process(p, buf)
        L.nut_buffer_free(buf)
        want_mask = c.add(rows, mask=True)
        assert np.array_equal(want_mask, R.detect(rows, 1, 9, 45, R.SO))
        assert np.array_equal(duty(), c.hits().astype(np.float64) / c.rows), k
        assert np.array_equal(mask().reshape(-1, N), want_mask), k
    short = L.nut_buffer_new_u8(N - 1, 2, block.ctypes.data)                     # shorter than a frame: nothing is added
    L.nrf_spectrum_occupancy_process(p, short)
    L.nut_buffer_free(short)
    assert np.array_equal(duty(), c.hits().astype(np.float64) / c.rows) and mask().size == 0
    L.nrf_spectrum_occupancy_free(p)
    c.close()


def test_host_block_refuses_an_f64_buffer():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from frequensea_amd import nrf\n"
            "L = nrf.nrf_lib()\n"
            "p = L.nrf_spectrum_occupancy_new(128, 128, 2, 16, 60, 0)\n"
            "L.nrf_spectrum_occupancy_process(p, L.nut_buffer_new_f64(4096, 2, None))\n"
            "print('returned')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "NRF SPECTRUM OCCUPANCY fatal error" in r.stderr and "F64" in r.stderr
