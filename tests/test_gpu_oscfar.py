"""GPU tier: the ordered-statistic CFAR detector (fsea_oscfar_*, kernels fsea_oscfar_u8 / fsea_oscfar_f32 and their
element-wise forms) and the tools' --rank option.

Every comparison is bit for bit against tests/oscfar_ref.py applied to the very rows given to the object: mask, row hits,
hits and rows are integers and do not depend on the order of the additions, so there is no tolerance anywhere.  The device
form's outputs are tests/guarded.py payloads of exactly the documented size: a store outside them dirties a band.  The host
form packs its rows at a pitch of whole 16-byte groups (the 16-byte kernels); the device form with a pitch that is no multiple
of 16 bytes runs the element-wise kernels."""
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from oracle import oracle as O
from tests import cfar_ref as C
from tests import oscfar_ref as R
from tests.conftest import ROOT
from tests.guarded import Guarded
from tests.test_gpu_cfar import device_run, f32_special_rows

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "frequensea_amd", "bin")
TILE, RUN = fsea.OSCFAR_TILE_COLUMNS, fsea.OSCFAR_RUN_ROWS
LIMIT = 1 << 20
SMALL, WIDE = (2, 16, 24), (64, 256, 384)                       # (G, T, R): the default and the widest window
SETTINGS = [(0, 1, 1), (0, 1, 2), (2, 16, 1), (2, 16, 24), (2, 16, 32), (64, 256, 1), (64, 256, 384), (64, 256, 512)]
WIDTHS = sorted({1, 2, 15, 16, 17, TILE - 1, TILE, TILE + 1} | {w for G, T, _ in (SMALL, WIDE) for w in (G + T, G + T + 1, 2 * TILE + G + T + 1)})


def check(c, rows, gtr, offset, what="", host=True, **kw):
    """Device form (guarded) and host form against the restatement; returns the expected mask."""
    G, T, rank = gtr
    c.set(G, T, offset, rank)
    want = R.detect(rows, G, T, offset, rank)
    m, h, hits, n = device_run(c, rows, **kw)
    assert np.array_equal(m, want), (what, "mask", int((m != want).sum()), np.argwhere(m != want)[:4].tolist())
    assert np.array_equal(h, C.row_hits_of(want)), (what, "row hits")
    assert np.array_equal(hits, C.hits_of(want)) and n == rows.shape[0], (what, "hits")
    if host:
        c.reset()
        hm, hh = c.add(rows, mask=True, row_hits=True)
        assert np.array_equal(hm, want) and np.array_equal(hh, C.row_hits_of(want)), (what, "host form")
        assert np.array_equal(c.hits(), C.hits_of(want)) and c.rows == rows.shape[0], (what, "host form hits")
    return want


@pytest.mark.parametrize("width", WIDTHS)
def test_widths(width):
    """u8 and f32 rows at every width with the default and the widest window: one cell, a width below the halo (every window
    clipped), the tile and its neighbours, and 2 C + G + T + 1, where a halo spans a whole tile seam and the last tile is
    one cell past it.  pitch = width (the 16-byte kernel where width is a multiple of 16) and width + 5 (element-wise)."""
    rng = np.random.default_rng(width)
    rows = rng.integers(0, 256, (3, width), dtype=np.uint8)
    f32 = f32_special_rows(width, 2, width)
    c = fsea.OsCfar(width)
    assert c.width == width and c.rows == 0 and c.rank == 24 and not c.hits().any()
    some = False
    for gtr in (SMALL, WIDE):
        some |= check(c, rows, gtr, 20, what=(width, gtr)).any()
        check(c, rows, gtr, 20, pitch=width + 5, lead=32, fence=0xFF, host=False, what=(width, gtr, "element-wise"))
        check(c, f32, gtr, 6 * 64, what=(width, gtr, "f32"))
    assert width < 300 or some
    c.close()


@pytest.mark.parametrize("gtr", SETTINGS)
def test_settings(gtr):
    """Every setting at width 17 and at its own 2 C + G + T + 1: rank 1 (the minimum), the default, rank 2T (the maximum),
    the smallest window and the widest."""
    G, T, rank = gtr
    for width in (17, 2 * TILE + G + T + 1):
        rows = np.random.default_rng(width).integers(0, 256, (3, width), dtype=np.uint8)
        c = fsea.OsCfar(width)
        want = check(c, rows, gtr, 10, what=(width, gtr))
        assert not want.all() and (want.any() or T == 256)        # no byte stands 10 above the largest of 512, and at width 17
                                                                  # the widest window has no cell inside the row
        check(c, rows, gtr, 10, pitch=width + 3, host=False, what=(width, gtr, "element-wise"))
        c.close()


@pytest.mark.parametrize("n", [1, RUN - 1, RUN, RUN + 1, 2 * RUN + 2])
def test_row_counts(n):
    width = TILE + 1
    rows = np.random.default_rng(n).integers(0, 256, (n, width), dtype=np.uint8)
    c = fsea.OsCfar(width)
    assert check(c, rows, SMALL, 20, what=n).any()
    c.close()


@pytest.mark.parametrize("offset", [60, 0, -1, -LIMIT, LIMIT])
def test_offsets(offset):
    """u8 rows and f32 rows with NaN, +-inf, values beyond both clamps and halves that round to even at 1/64 dB, at the
    offsets' ends.  At -2^20 every cell with a training cell inside the row is a hit unless the r-th level stands 2^20 above
    it; at 2^20 none is: the level given to the cells outside a row must hold at both."""
    width = TILE + 37
    rows = np.random.default_rng(4).integers(0, 256, (3, width), dtype=np.uint8)
    f32 = f32_special_rows(width, 3, 4)
    lv = C.levels_of_f32(f32)
    assert {-LIMIT, LIMIT} <= set(lv.ravel().tolist()) and np.isnan(f32).any()
    assert C.levels_of_f32(np.array([0.5 / 64, 1.5 / 64, 2.5 / 64, -0.5 / 64, -1.5 / 64], np.float32)).tolist() == [0, 2, 2, 0, -2]
    c = fsea.OsCfar(width)
    for gtr in (SMALL, (0, 3, 1), WIDE):
        u = check(c, rows, gtr, offset, what=("u8", gtr, offset))
        f = check(c, f32, gtr, offset if abs(offset) == LIMIT else offset * 64, what=("f32", gtr, offset))
        if offset == -LIMIT:
            assert u.all() and f.any()
        if offset == LIMIT:
            assert not u.any()                                     # f32: only a cell at 2^20 over an r-th level of -2^20
    check(c, f32, SMALL, 640, pitch=width + 3, lead=4, fence=0xFF, host=False, what="f32 element-wise")        # 0xFF: NaNs
    check(c, f32, SMALL, 640, pitch=(width + 3) // 4 * 4 + 4, lead=8, host=False, what="f32 partial group")
    c.close()


def test_rows_of_few_levels():
    """Ties decide: three levels, two levels and a constant row, at the offsets where `>` and `>=` part."""
    width = TILE + 100
    rng = np.random.default_rng(6)
    rows = np.stack([100 + rng.integers(0, 3, width), 7 * rng.integers(0, 2, width), np.full(width, 255), np.zeros(width, np.int64),
                     100 + (rng.random(width) < 0.05)]).astype(np.uint8)
    c = fsea.OsCfar(width)
    for gtr in (SMALL, (2, 16, 1), (2, 16, 32), (1, 3, 4), WIDE):
        for offset in (0, -1, 1):
            want = check(c, rows, gtr, offset, what=(gtr, offset), host=False)
            assert want[2:4].all() if offset == -1 else not want[2:4].any()      # the constant rows: x > x + offset
    c.close()


def test_pitches_and_a_sub_band_of_wider_rows():
    """A pitch that is no multiple of 16 bytes, a width that is no multiple of 16 (the byte-wise mask), and columns 16 j ..
    of rows 1504 wide (16-byte kernel) and 1500 wide (element-wise); the fence round the rows does not move the result."""
    rng = np.random.default_rng(5)
    for wide_w, width, j in ((1504, 1100, 3), (1500, 1100, 3), (1504, 7, 1), (2400, 1040, 5)):
        wide = rng.integers(0, 256, (9, wide_w), dtype=np.uint8)
        band = wide[:, 16 * j:16 * j + width]
        c = fsea.OsCfar(width)
        for gtr in (SMALL, WIDE):
            c.set(gtr[0], gtr[1], 20, gtr[2])
            c.reset()
            want = R.detect(band, gtr[0], gtr[1], 20, gtr[2])
            buf = fsea.DeviceBuffer(wide.nbytes).upload(wide)
            g_mask = Guarded(band.size)
            c.add_device(buf.ptr.value + 16 * j, fsea.CFAR_U8, 9, wide_w, g_mask.addr)
            assert np.array_equal(c.hits(), C.hits_of(want)), (wide_w, width, gtr)
            assert np.array_equal(g_mask.payload(np.uint8, band.shape), want), (wide_w, width, gtr)
            g_mask.check("mask of a sub-band")
            g_mask.free()
            buf.free()
        c.close()
    width = TILE - 3
    rows = rng.integers(0, 256, (4, width), dtype=np.uint8)
    c = fsea.OsCfar(width)
    for pitch in (width, width + 3, width + 19):
        for fence in (0x00, 0xFF):
            check(c, rows, WIDE, 10, pitch=pitch, lead=16, fence=fence, host=False, what=(pitch, fence))
    c.close()


def test_cuts_streams_optional_outputs_and_reset():
    width, n = TILE + 100, 2 * RUN + 7
    rows = np.random.default_rng(8).integers(0, 256, (n, width), dtype=np.uint8)
    gtr, offset = (3, 9, 12), 25
    want = R.detect(rows, gtr[0], gtr[1], offset, gtr[2])
    c = fsea.OsCfar(width)
    c.set(gtr[0], gtr[1], offset, gtr[2])
    assert c.rank == 12
    # the same rows in one call, and cut at 1, RUN - 1 and RUN + 3 rows on two streams: the same hits and rows
    c.add(rows)
    assert np.array_equal(c.hits(), C.hits_of(want)) and c.rows == n
    c.reset()
    s = (fsea.Stream(), fsea.Stream())
    d_rows = fsea.DeviceBuffer(rows.nbytes).upload(rows)
    cuts = [0, 1, RUN - 1, RUN + 3, n]
    assert width % 16 != 0                                                        # the parts' bases are not all aligned ...
    parts = []
    for i in range(4):
        a, b = cuts[i], cuts[i + 1]
        part = fsea.DeviceBuffer(max(1, b - a) * width).upload(rows[a:b])       # ... so each part goes up on its own
        g_mask = Guarded((b - a) * width)
        c.add_device(part.ptr.value, fsea.CFAR_U8, b - a, width, g_mask.addr, stream=s[i & 1])
        parts.append((a, b, part, g_mask))
    c.add_device(d_rows.ptr.value, fsea.CFAR_U8, n, width, stream=s[0])          # no mask, no wait in between
    assert np.array_equal(c.hits(), 2 * C.hits_of(want)) and c.rows == 2 * n     # hits(): behind every add, whatever its stream
    for a, b, part, g_mask in parts:
        assert np.array_equal(g_mask.payload(np.uint8, (b - a, width)), want[a:b]), (a, b)
        g_mask.check("mask of a part")
        g_mask.free()
        part.free()
    # row_hits is set, not added to: twice into the same buffer
    g_hits = Guarded(4 * n).upload(np.full(n, 0xDEADBEEF, np.uint32))
    for _ in range(2):
        c.add_device(d_rows.ptr.value, fsea.CFAR_U8, n, width, None, g_hits.addr)
    assert np.array_equal(g_hits.payload(np.uint32, (n,)), C.row_hits_of(want)) and c.rows == 4 * n
    g_hits.check("row hits")
    g_hits.free()
    # the optional outputs of both forms
    m, h, hits, _ = device_run(c, rows[:7], mask=True, row_hits=False)
    assert h is None and np.array_equal(m, want[:7]) and np.array_equal(hits, C.hits_of(want[:7]))
    m, h, hits, total = device_run(c, rows[:7], mask=False, row_hits=True, reset=False)
    assert m is None and np.array_equal(h, C.row_hits_of(want[:7])) and np.array_equal(hits, 2 * C.hits_of(want[:7])) and total == 14
    assert c.add(rows[:7]) is None and c.rows == 21
    assert np.array_equal(c.add(rows[:7], row_hits=True), C.row_hits_of(want[:7]))
    c.add(rows[:0])                                                               # no rows: a successful no-op
    c.add_device(0, fsea.CFAR_U8, 0, width)
    assert c.rows == 28
    c.reset()                                                                     # zeroes hits and rows, keeps the four settings
    assert c.rows == 0 and not c.hits().any() and c.rank == 12
    assert np.array_equal(c.add(rows, mask=True), want)                           # add_host equals add_device
    d_rows.free()
    for o in s + (c,):
        o.close()
    for _ in range(10):                                                           # create / destroy cycles
        c = fsea.OsCfar(64)
        c.add(rows[:2, :64])
        c.close()


def test_the_worked_case_beside_cfar():
    """A row of 128 cells at 100, a carrier of 200 on 40 .. 47 and one of 130 on 60; G = 2, T = 16, offset 20: CA misses
    column 60, rank 24 of 32 finds it."""
    row = np.full((1, 128), 100, np.uint8)
    row[0, 40:48] = 200
    row[0, 60] = 130
    ca, os_ = fsea.Cfar(128), fsea.OsCfar(128)
    ca.set(2, 16, 20, fsea.CFAR_CA)
    os_.set(2, 16, 20, 24)
    m_ca, m_os = ca.add(row, mask=True), os_.add(row, mask=True)
    assert np.flatnonzero(m_ca[0]).tolist() == list(range(40, 48))
    assert np.flatnonzero(m_os[0]).tolist() == list(range(40, 48)) + [60]
    assert np.array_equal(m_os, R.detect(row, 2, 16, 20, 24)) and os_.hits()[60] == 1 and ca.hits()[60] == 0
    ca.close()
    os_.close()


# Two tones 12 bins and 25 dB apart in a 64-point DB5 row: amplitudes 122 and 122 / 10^(25/20) on bins +8 and +20, noise of
# sigma 0.25.  The oracle's rows hold them at levels 148 and 21 .. 22 over a floor of 0.  At (2, 16, offset 19) the weaker
# one sees a mean of 148 / 32 = 4.6 and would need more than 23.6 under CA; the 24th smallest of its 32 neighbours is 0.
N2, FRAMES2, STRONG, WEAK, OFFSET2 = 64, 40, 32 + 8, 32 + 20, 19


def two_tones():
    rng = np.random.default_rng(1)
    t = np.arange(N2 * FRAMES2)
    a1 = 122.0
    z = a1 * np.exp(2j * np.pi * 8 * t / N2) + a1 / 10 ** (25 / 20) * np.exp(2j * np.pi * (20 * t / N2 + 0.3))
    z = z + rng.normal(0, 0.25, t.size) + 1j * rng.normal(0, 0.25, t.size)
    iq = np.empty(2 * t.size, np.int8)
    iq[0::2] = np.clip(np.rint(z.real), -127, 127)
    iq[1::2] = np.clip(np.rint(z.imag), -127, 127)
    return iq.view(np.uint8)


def test_through_the_chain_into_events():
    raw = two_tones()
    # on the CPU first: the oracle's rows through the two restatements
    rows_cpu = O.rows(raw, FRAMES2, N2, mode=O.MODE_DB5_U8_DCFIX)
    ca_cpu, os_cpu = C.detect(rows_cpu, 2, 16, OFFSET2, C.CA), R.detect(rows_cpu, 2, 16, OFFSET2, 24)
    assert ca_cpu[:, STRONG].all() and os_cpu[:, STRONG].all() and os_cpu[:, WEAK].all() and not ca_cpu[:, WEAK].any()
    # on the device: plan -> detector -> events, no row visits the host in between
    plan = fsea.Plan(N2, N2, fsea.MODE_DB5_U8_DCFIX)
    d_iq = fsea.DeviceBuffer(raw.nbytes).upload(raw)
    d_rows = fsea.DeviceBuffer(FRAMES2 * N2)
    plan.exec_device(d_iq.ptr.value, FRAMES2, d_rows.ptr.value, flip=True)
    rows = d_rows.download(np.uint8, (FRAMES2, N2))
    found = {}
    for name, det, want in (("os", fsea.OsCfar(N2), R.detect(rows, 2, 16, OFFSET2, 24)), ("ca", fsea.Cfar(N2), C.detect(rows, 2, 16, OFFSET2, C.CA))):
        det.set(2, 16, OFFSET2, 24 if name == "os" else fsea.CFAR_CA)
        g_mask = Guarded(FRAMES2 * N2)
        det.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES2, N2, g_mask.addr)
        assert np.array_equal(g_mask.payload(np.uint8, (FRAMES2, N2)), want), name
        g_mask.check("mask")
        ev = fsea.Events(N2)
        d_runs = fsea.DeviceBuffer(FRAMES2 * N2 * fsea.EVENTS_RUN.itemsize)
        n = ev.runs_device(g_mask.addr, FRAMES2, d_runs.ptr.value, FRAMES2 * N2, d_levels_ptr=d_rows.ptr.value)
        runs = d_runs.download(fsea.EVENTS_RUN, (n,))
        found[name] = [(int(r["row"]), int(r["first"]), int(r["last"])) for r in runs]
        for o in (g_mask, d_runs):
            o.free()
        for o in (ev, det):
            o.close()
    weak = [(row, WEAK, WEAK) for row in range(FRAMES2)]
    strong = [(row, STRONG, STRONG) for row in range(FRAMES2)]
    assert found["os"] == sorted(strong + weak)                  # the weaker tone's run is there in every row ...
    assert found["ca"] == strong                                 # ... and absent under CA at the same (G, T, offset)
    plan.close()
    d_iq.free()
    d_rows.free()


def _plan_rows(raw):
    plan = fsea.Plan(N2, N2, fsea.MODE_DB5_U8_DCFIX)
    rows = plan.exec_host(raw, FRAMES2, flip=True)
    plan.close()
    return rows


def test_occupancy_tool_with_a_rank(tmp_path):
    from PIL import Image
    raw = two_tones()
    raw.tofile(tmp_path / "tones.raw")
    rows = _plan_rows(raw)
    want = R.detect(rows, 2, 16, OFFSET2, 24)
    bands = C.bands_of(C.hits_of(want), FRAMES2, 0.5, 0, 1)
    assert [(int(b["first"]), int(b["last"])) for b in bands] == [(STRONG, STRONG), (WEAK, WEAK)]
    lines = ["%d %d %d %.6f" % (b["first"], b["last"], b["peak"], b["peak_hits"] / FRAMES2) for b in bands]
    tool = os.path.join(BIN, "fsea-occupancy")
    out, bands_path = tmp_path / "mask.png", tmp_path / "bands.txt"
    Image.fromarray(rows).save(tmp_path / "rows.png")
    for source in ([str(tmp_path / "tones.raw"), "--size", str(N2), "--flip"], ["--image", str(tmp_path / "rows.png")]):
        r = subprocess.run([tool] + source + ["--offset", str(OFFSET2), "--rank", "24", "--mask", str(out), "--bands", str(bands_path)],
                           capture_output=True, text=True, check=True, timeout=300)
        assert r.stdout.split("\n")[:1 + len(lines)] == ["rows %d" % FRAMES2] + lines, source
        assert open(bands_path).read().split("\n") == lines + [""]
        with Image.open(out) as im:
            got = np.array(im)
        assert got.dtype == np.uint8 and np.array_equal(got, want), source
        os.remove(out)
    # without --rank: the mean, which misses the weaker tone
    r = subprocess.run([tool, str(tmp_path / "tones.raw"), "--size", str(N2), "--flip", "--offset", str(OFFSET2)], capture_output=True,
                       text=True, check=True, timeout=300)
    assert r.stdout.split("\n")[:3] == ["rows %d" % FRAMES2, lines[0], ""]


def test_events_and_cutouts_tools_with_a_rank(tmp_path):
    raw = two_tones()
    raw.tofile(tmp_path / "tones.raw")
    head = [str(tmp_path / "tones.raw"), "--size", str(N2), "--flip", "--offset", str(OFFSET2)]
    tool = os.path.join(BIN, "fsea-events")
    boxes = {}
    for name, more in (("os", ["--rank", "24"]), ("ca", [])):
        r = subprocess.run([tool] + head + more, capture_output=True, text=True, check=True, timeout=300)
        lines = r.stdout.split("\n")
        boxes[name] = [tuple(int(v) for v in line.split()[:4]) for line in lines[1:] if line]
        assert lines[0] == "rows %d runs %d events %d" % (FRAMES2, FRAMES2 * len(boxes[name]), len(boxes[name])), (name, lines[0])
    assert boxes["os"] == [(0, FRAMES2 - 1, STRONG, STRONG), (0, FRAMES2 - 1, WEAK, WEAK)]        # the weaker emission is reported
    assert boxes["ca"] == [(0, FRAMES2 - 1, STRONG, STRONG)]
    out = tmp_path / "cut"
    r = subprocess.run([os.path.join(BIN, "fsea-cutouts")] + head + ["--rank", "24", "--decimation", "4", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "rows %d runs %d events 2 cutouts 2 skipped 0\n" % (FRAMES2, 2 * FRAMES2)
    lines = open(out / "cutouts.txt").read().split("\n")
    assert [tuple(int(v) for v in line.split()[:5]) for line in lines if line] == [(0, 0, FRAMES2 - 1, STRONG, STRONG), (1, 0, FRAMES2 - 1, WEAK, WEAK)]
    assert sorted(f for f in os.listdir(out) if f.endswith(".cf32")) == ["cutout-00000.cf32", "cutout-00001.cf32"]
