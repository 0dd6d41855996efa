"""GPU tier: the time-axis CFAR detector (fsea_tcfar_*, kernels fsea_tcfar_u8 / fsea_tcfar_f32 and their element-wise forms)
and --axis time|either of fsea-occupancy, fsea-events and fsea-cutouts.

Every comparison is bit for bit against tests/tcfar_ref.py (the header's one sentence: fsea_cfar's restatement on the
transposed block) applied to the very rows given to the object: mask, row hits, hits and rows are integers and depend on
neither the launch geometry nor the cut into calls, so there is no tolerance anywhere.  The device form's outputs are
tests/guarded.py payloads of exactly the documented size: a store outside them dirties a band.  The host form packs its rows
at a pitch of whole 16-byte groups (the 16-byte kernels); the device form with a pitch that is no multiple of 16 bytes runs
the element-wise kernels.  Seams are read from fsea.Tcfar.run_rows under the settings in force and TCFAR_TILE_COLUMNS."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import cfar_ref as R
from tests import events_ref as E
from tests import tcfar_ref as TR
from tests.conftest import ROOT, synth_iq
from tests.guarded import Guarded
from tests.test_gpu_cfar import f32_special_rows
from tests.test_gpu_events import event_lines

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "frequensea_amd", "bin")
TILE = fsea.TCFAR_TILE_COLUMNS
DEFAULT = (2, 16, 60, R.CA)
GARBAGE = 0xDEADBEEF


def run_rows(settings=DEFAULT):
    c = fsea.Tcfar(16)
    c.set(*settings)
    run = c.run_rows
    c.close()
    assert run >= 1
    return run


RUN = None      # run_rows(DEFAULT), asked once a test needs it: no device at import


def default_run():
    global RUN
    if RUN is None:
        RUN = run_rows()
    return RUN


def device_run(c, block, before=0, after=0, pitch=None, lead=0, fence=0x00, mask=True, row_hits=True, stream=0, reset=True):
    """One add_device that decides rows before .. len(block) - after - 1 of `block`, laid out `pitch` elements apart, `lead`
    elements (a multiple of 16 bytes) behind the start of a buffer otherwise full of `fence` bytes, between guard bands of
    the same; the lead grows by up to 15 bytes where the first decided row would not begin at a 16-byte boundary, as the
    device form asks.  Mask and row hits go into guarded payloads of exactly n * width bytes and n uint32.  `mask`: True
    (pre-filled with the guard's fill), False, or an (n, width) uint8 array the payload starts as.  Returns (mask, row_hits,
    hits, rows)."""
    total, width = block.shape
    n = total - before - after
    pitch = width if pitch is None else pitch
    lead += -(lead + before * pitch) % (16 // block.itemsize)
    flat = np.full((lead + max(total, 1) * pitch) * block.itemsize, fence, np.uint8).view(block.dtype).copy()
    for r in range(total):
        flat[lead + r * pitch: lead + r * pitch + width] = block[r]
    g_in = Guarded(flat.nbytes, fill=fence).upload(flat)
    want_mask = mask is not False
    g_mask = Guarded(n * width) if want_mask else None
    if isinstance(mask, np.ndarray):
        g_mask.upload(mask)
    g_hits = Guarded(4 * n) if row_hits else None
    if row_hits and n:
        g_hits.upload(np.full(n, GARBAGE, np.uint32))
    if reset:
        c.reset()
    c.add_device(g_in.addr + (lead + before * pitch) * block.itemsize, fsea.CFAR_U8 if block.dtype == np.uint8 else fsea.CFAR_F32, n,
                 pitch, before, after, g_mask.addr if want_mask else None, g_hits.addr if row_hits else None, stream=stream)
    hits = c.hits()                                            # behind the add, whatever its stream
    got_mask = g_mask.payload(np.uint8, (n, width)) if want_mask else None
    got_hits = g_hits.payload(np.uint32, (n,)) if row_hits else None
    for g, what in ((g_mask, "mask"), (g_hits, "row hits"), (g_in, "input")):
        if g is not None:
            g.check(what)
            g.free()
    return got_mask, got_hits, hits, c.rows


def check(c, block, settings=DEFAULT, before=0, after=0, what="", host=True, **kw):
    """Device form (guarded) and host form against the restatement; returns the expected mask."""
    c.set(*settings)
    n = block.shape[0] - before - after
    want = TR.detect(block, before, n, *settings)
    m, h, hits, rows = device_run(c, block, before, after, **kw)
    assert np.array_equal(m, want), (what, "mask", int((m != want).sum()), np.argwhere(m != want)[:4].tolist())
    assert np.array_equal(h, R.row_hits_of(want)), (what, "row hits")
    assert np.array_equal(hits, R.hits_of(want)) and rows == n, (what, "hits")
    if host:
        c.reset()
        hm, hh = c.add(block, before, after, mask=True, row_hits=True)
        assert np.array_equal(hm, want) and np.array_equal(hh, R.row_hits_of(want)), (what, "host form")
        assert np.array_equal(c.hits(), R.hits_of(want)) and c.rows == n, (what, "host form hits")
    return want


def row_counts(G, T, run):
    return sorted({1, 2, G + T, G + T + 1, 2 * (G + T) + 1, run - 1, run, run + 1, 2 * run + 3} - {0})


@pytest.mark.parametrize("width", [1, 2, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_random_u8_rows(width):
    """Random bytes near one level with single cells and whole rows far above it (among full-range bytes hardly one stands 60
    above the mean of 32); every row count at which a window is whole, clipped or across a run seam, no context; pitch = width and width + 5 (the
    element-wise kernel) and, at a multiple of 16 above the width behind a 32-byte lead, the 16-byte kernel on rows whose
    last group is partial, in a buffer fenced with 0xFF."""
    run = default_run()
    rng = np.random.default_rng(width)
    rows = rng.integers(90, 110, (2 * run + 3, width), dtype=np.uint8)
    rows[rng.random(rows.shape) < 0.05] = 200
    rows[rng.integers(0, rows.shape[0], 6)] += 70              # whole rows: wide bursts
    c = fsea.Tcfar(width)
    assert c.width == width and c.rows == 0 and not c.hits().any() and c.run_rows == run
    any_hit = False
    for n in row_counts(2, 16, run):
        any_hit |= bool(check(c, rows[:n], what=(width, n)).any())
    assert any_hit
    for pitch in (width + 5, (width + 15) // 16 * 16 + 16):
        check(c, rows[:run + 1], pitch=pitch, lead=32, fence=0xFF, host=False, what=(width, "pitch", pitch))
    c.close()


@pytest.mark.parametrize("width", [1, 3, 4, 50, TILE + 5])
def test_f32_rows(width):
    """dB values with every clamp, NaN and half-way ties; the three methods; offsets +-2^20 against levels at both clamps (the
    32-bit bound: |x n - S - offset n| reaches 3 * 2^28); the element-wise kernel and a partial last group."""
    run = default_run()
    rows = f32_special_rows(width, run + 2, width)
    rows[5] = 1e9                                              # a row at the upper clamp, one at the lower
    rows[9] = -1e9
    c = fsea.Tcfar(width)
    for settings in ((2, 16, 60 * 64, R.CA), (1, 5, 0, R.GO), (0, 3, -(1 << 20), R.SO), (64, 256, 1 << 20, R.CA), (0, 256, -(1 << 20), R.GO),
                     (0, 4, 1 << 20, R.SO)):
        check(c, rows, settings, what=(width, settings))
    check(c, rows[:7], (2, 16, 640, R.SO), pitch=width + 3, lead=4, fence=0xFF, host=False, what=(width, "element-wise"))   # 0xFF: NaNs
    check(c, rows[:7], (2, 16, 640, R.CA), pitch=(width + 3) // 4 * 4 + 4, lead=8, host=False, what=(width, "partial group"))
    c.close()


@pytest.mark.parametrize("width", [7, TILE + 700])
@pytest.mark.parametrize("method", [R.CA, R.GO, R.SO])
def test_the_widest_windows(width, method):
    """(64, 256) on 5 rows, where every window is clipped or empty, and on 2 RUN + 3 rows, where windows reach across a run
    seam."""
    settings = (64, 256, 3, method)
    run = run_rows(settings)
    rng = np.random.default_rng(width)
    rows = rng.integers(95, 106, (2 * run + 3, width), dtype=np.uint8)
    rows[run - 2: run + 3] += 40
    c = fsea.Tcfar(width)
    assert not check(c, rows[:5], settings, what=(width, 5)).any()                 # fewer than G + 2 rows: no training row
    assert check(c, rows, settings, what=(width, "seam")).any()
    check(c, rows, settings, pitch=width + 5, host=False, what=(width, "element-wise"))
    c.close()


@pytest.mark.parametrize("settings", [DEFAULT, (0, 1, 10, R.SO), (3, 7, -3, R.GO)])
def test_context_rows(settings):
    """The middle of a block of 3 RUN + 7 rows, with none, some, exactly G + T and G + T + 9 rows of context on each side:
    the windows end where the call's rows end, and context beyond G + T changes nothing."""
    run = run_rows(settings)
    reach = settings[0] + settings[1]
    width = TILE + 21
    rng = np.random.default_rng(reach)
    block = rng.integers(90, 110, (3 * run + 7, width), dtype=np.uint8)
    block[rng.integers(0, block.shape[0], 12)] += 60
    first, n = run + 3, run + 2
    c = fsea.Tcfar(width)
    masks = {}
    for before in sorted({0, max(reach // 2, 1) if reach > 1 else 0, reach, reach + 9}):
        for after in sorted({0, max(reach // 2, 1) if reach > 1 else 0, reach, reach + 9}):
            part = block[first - before: first + n + after]
            masks[before, after] = check(c, part, settings, before, after, host=(before == after), what=(settings, before, after))
    whole = TR.detect(block, 0, block.shape[0], *settings)[first:first + n]
    assert np.array_equal(masks[reach, reach], whole) and np.array_equal(masks[reach + 9, reach + 9], whole)
    assert not np.array_equal(masks[0, 0], whole)
    c.close()


def test_cut_invariance():
    """One block in one call, and in calls of 1, RUN - 1, RUN + 1 rows and the rest, each with min(G + T, available) rows of
    context: the concatenated masks and the final hits are those of the one call; device and host form."""
    run = default_run()
    width, total, reach = TILE + 100, 3 * run + 7, 18
    rng = np.random.default_rng(8)
    block = rng.integers(90, 110, (total, width), dtype=np.uint8)
    block[rng.integers(0, total, 10)] += 60
    want = TR.detect(block, 0, total, *DEFAULT)
    c = fsea.Tcfar(width)
    c.set(*DEFAULT)
    assert np.array_equal(c.add(block, mask=True), want) and np.array_equal(c.hits(), R.hits_of(want)) and c.rows == total
    cuts, first = [], 0
    for n in (1, run - 1, run + 1, total - 2 * run - 1):
        cuts.append((first, n))
        first += n
    assert first == total
    for host in (True, False):
        c.reset()
        parts = []
        for first, n in cuts:
            before, after = TR.context(total, first, n, reach)
            part = block[first - before: first + n + after]
            if host:
                parts.append(c.add(part, before, after, mask=True))
            else:
                parts.append(device_run(c, part, before, after, reset=False)[0])
        assert np.array_equal(np.concatenate(parts), want), host
        assert np.array_equal(c.hits(), R.hits_of(want)) and c.rows == total, host
    c.close()


def test_a_sub_band_of_wider_rows():
    """Columns 48 .. 48 + width of rows 1500 wide, on the device at the wide pitch (1504: the 16-byte kernel; 1500:
    element-wise) between context rows, and from a host array with an odd base."""
    rng = np.random.default_rng(5)
    for wide_w, width in ((1504, 1100), (1500, 1100), (1504, 7)):
        wide = rng.integers(90, 110, (40, wide_w), dtype=np.uint8)
        wide[rng.integers(0, 40, 4)] += 70
        band = wide[:, 48:48 + width]
        want = TR.detect(band, 16, 20, *DEFAULT)                # 16 rows of context: the first decided row is aligned
        buf = fsea.DeviceBuffer(wide.nbytes).upload(wide)
        g_mask = Guarded(20 * width)
        c = fsea.Tcfar(width)
        c.add_device(buf.ptr.value + 16 * wide_w + 48, fsea.CFAR_U8, 20, wide_w, 16, 4, g_mask.addr)
        assert np.array_equal(c.hits(), R.hits_of(want)), (wide_w, width)
        assert np.array_equal(g_mask.payload(np.uint8, (20, width)), want) and want.any()
        g_mask.check("mask of a sub-band")
        odd = wide[:, 3:3 + width] if wide.ctypes.data % 2 == 0 else wide[:, 4:4 + width]
        c.reset()
        assert np.array_equal(c.add(odd, 16, 4, mask=True), TR.detect(odd, 16, 20, *DEFAULT))
        c.close()
        g_mask.free()
        buf.free()


@pytest.mark.parametrize("width", [16 * 9, 16 * 9 + 5])
def test_mask_operations(width):
    """A mask first written by fsea.Cfar on the same rows, then OR and AND; a mask prefilled with bytes 0, 1, 7 and 255.
    Mask, row hits and hits describe the written value."""
    run = default_run()
    rng = np.random.default_rng(width)
    rows = rng.integers(95, 106, (run + 5, width), dtype=np.uint8)
    rows[20:26, 8:width - 8] += 60                             # a wide burst: the time axis fills what the frequency axis leaves
    rows[:, 3] = 200                                           # a carrier: the frequency axis alone
    settings = (2, 16, 20, R.CA)
    freq = fsea.Cfar(width)
    freq.set(*settings)
    across = freq.add(rows, mask=True)
    freq.close()
    assert np.array_equal(across, R.detect(rows, *settings))
    down = TR.detect(rows, 0, rows.shape[0], *settings)
    assert down[20:26, 8:width - 8].all() and not down[:, 3].any() and across[:, 3].all() and not across[22, 30:width - 30].any()
    prefilled = rng.choice(np.array([0, 1, 7, 255], np.uint8), rows.shape)
    c = fsea.Tcfar(width)
    for old in (across, prefilled):
        for op in (TR.MASK_SET, TR.MASK_OR, TR.MASK_AND):
            c.set(*settings, op)
            want = TR.combine(old, down, op)
            m, h, hits, n = device_run(c, rows, mask=old)
            assert np.array_equal(m, want) and np.array_equal(h, R.row_hits_of(want)), (width, op)
            assert np.array_equal(hits, R.hits_of(want)) and n == rows.shape[0], (width, op)
            c.reset()
            inout = old.copy()
            hm, hh = c.add(rows, mask=inout, row_hits=True)
            assert hm is inout and np.array_equal(inout, want) and np.array_equal(hh, R.row_hits_of(want)), (width, op, "host form")
            assert np.array_equal(c.hits(), R.hits_of(want)), (width, op, "host form hits")
    both = TR.combine(across, down, TR.MASK_AND)
    assert both.any() and not np.array_equal(both, down) and not np.array_equal(TR.combine(across, down, TR.MASK_OR), down)
    # OR without a mask is refused and leaves the object unchanged
    c.set(*settings, TR.MASK_OR)
    c.reset()
    d_rows = fsea.DeviceBuffer(rows.nbytes).upload(rows)
    with pytest.raises(fsea.FseaError, match="combines with a mask"):
        c.add_device(d_rows.ptr.value, fsea.CFAR_U8, rows.shape[0], width)
    with pytest.raises(fsea.FseaError, match="combines with a mask"):
        c.add(rows)
    assert c.rows == 0 and not c.hits().any()
    d_rows.free()
    c.close()


def test_the_object():
    """Two adds on two streams with the hits read after both; reset keeps the settings; n_rows == 0; optional outputs; the
    2^32 - 1 rows guard through a `rows` value written into the object."""
    run = default_run()
    width, n = TILE + 100, run + 9
    rows = np.random.default_rng(9).integers(90, 110, (n, width), dtype=np.uint8)
    rows[[7, 40, run + 2]] += 50
    settings = (1, 9, 30, R.GO)
    want = TR.detect(rows, 0, n, *settings)
    assert want.any()
    c = fsea.Tcfar(width)
    c.set(*settings)
    s1, s2 = fsea.Stream(), fsea.Stream()
    d_rows = fsea.DeviceBuffer(rows.nbytes).upload(rows)
    d_mask = fsea.DeviceBuffer(rows.nbytes)
    cut = 16
    assert (cut * width) % 16 == 0                                                        # the second part's base is aligned
    c.add_device(d_rows.ptr.value, fsea.CFAR_U8, cut, width, 0, n - cut, d_mask.ptr.value, stream=s1)
    c.add_device(d_rows.ptr.value + cut * width, fsea.CFAR_U8, n - cut, width, cut, 0, d_mask.ptr.value + cut * width, stream=s2)
    c.add_device(d_rows.ptr.value, fsea.CFAR_U8, n, width, stream=s1)                      # no wait in between
    assert np.array_equal(c.hits(), 2 * R.hits_of(want)) and c.rows == 2 * n
    assert np.array_equal(d_mask.download(np.uint8, rows.shape), want)
    c.reset()                                                                             # zeroes hits and rows, keeps the settings
    assert c.rows == 0 and not c.hits().any()
    assert np.array_equal(c.add(rows, mask=True), want)
    assert c.add(rows) is None and c.rows == 2 * n
    assert np.array_equal(c.add(rows, row_hits=True), R.row_hits_of(want))
    m, h, hits, total = device_run(c, rows, mask=False, row_hits=False, reset=False)
    assert m is None and h is None and np.array_equal(hits, 4 * R.hits_of(want)) and total == 4 * n
    c.add(rows[:0])                                                                       # no rows: a successful no-op
    c.add(rows[:5], before=2, after=3)                                                    # context alone
    c.add_device(0, fsea.CFAR_U8, 0, width)
    assert c.rows == 4 * n
    # rows would pass 2^32 - 1: the struct begins with int width, int device, uint64_t rows
    counter = ctypes.c_uint64.from_address(c._p.value + 8)
    assert counter.value == 4 * n
    counter.value = (1 << 32) - 3
    with pytest.raises(fsea.FseaError, match=r"past 2\^32 - 1"):
        c.add_device(d_rows.ptr.value, fsea.CFAR_U8, 3, width)
    with pytest.raises(fsea.FseaError, match=r"past 2\^32 - 1"):
        c.add(rows[:3])
    c.add_device(d_rows.ptr.value, fsea.CFAR_U8, 2, width)
    assert c.rows == (1 << 32) - 1
    counter.value = 0
    for o in (d_rows, d_mask):
        o.free()
    for o in (s1, s2, c):
        o.close()


def test_host_form_in_chunks_and_its_refusal():
    """f32 rows of 2^18 cells are 1 MiB each: 80 of them exceed one staging chunk of 64 MiB, so the host form goes in chunks
    of 64 - 2 * 18 = 28 rows, each with its context.  At (64, 256) the 641 rows of a decided row and its context do not fit:
    the host form refuses, the device form on the same rows succeeds."""
    width, n = 1 << 18, 80
    rng = np.random.default_rng(4)
    rows = rng.uniform(-100, -90, (n, width)).astype(np.float32)
    rows[[10, 27, 28, 55, 56, 79]] += 30.0                                                # at the chunk seams 28 and 56 among others
    settings = (2, 16, 10 * 64, R.CA)
    want = TR.detect(rows, 0, n, *settings)
    assert want[27].all() and want[28].all() and want[56].all()
    c = fsea.Tcfar(width)
    c.set(*settings)
    m, h = c.add(rows, mask=True, row_hits=True)
    assert np.array_equal(m, want) and np.array_equal(h, R.row_hits_of(want))
    assert np.array_equal(c.hits(), R.hits_of(want)) and c.rows == n
    wide = (64, 256, 10 * 64, R.CA)
    c.set(*wide)
    c.reset()
    with pytest.raises(fsea.FseaError, match="rows of 1048576 bytes: the 641 rows .* use fsea_tcfar_add_device"):
        c.add(rows, mask=True)
    assert c.rows == 0
    d_rows = fsea.DeviceBuffer(rows.nbytes).upload(rows)
    d_mask = fsea.DeviceBuffer(n * width)
    c.add_device(d_rows.ptr.value, fsea.CFAR_F32, n, width, d_mask_ptr=d_mask.ptr.value)
    wide_want = TR.detect(rows, 0, n, *wide)
    assert np.array_equal(d_mask.download(np.uint8, (n, width)), wide_want) and np.array_equal(c.hits(), R.hits_of(wide_want))
    assert wide_want.any()
    d_rows.free()
    d_mask.free()
    c.close()


# ---- the tools ------------------------------------------------------------------------------------------------------

N, HOP = 256, 256
CHUNK = ((1 << 22) - N) // HOP + 1          # frames of a tool's chunk (tools/tool_common.h)
FRAMES = CHUNK + 200
BURST = (CHUNK - 24, CHUNK - 11)            # rows of the wide burst: the seam between the chunks' own rows, CHUNK - 18, inside
EVENT_OPTIONS = ["--gap-cols", "2", "--gap-rows", "1", "--min-hits", "40"]
DETECTOR = (2, 16, 60, R.CA)


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """synth_iq's noise and tone with a wide burst, full-scale random signs (a flat spectrum some 15 dB above the noise),
    that straddles the seam of the tools' chunks; its rows through the plan, once."""
    assert CHUNK == 16384
    raw = synth_iq(3, 2 * N * FRAMES + 100).copy()                             # 50 samples over: no further frame
    loud = np.random.default_rng(4).choice(np.array([-120, 120], np.int8), 2 * N * (BURST[1] - BURST[0])).view(np.uint8)
    raw[2 * N * BURST[0]: 2 * N * BURST[1]] = loud
    path = tmp_path_factory.mktemp("tcfar") / "burst.raw"
    raw.tofile(path)
    plan = fsea.Plan(N, HOP, fsea.MODE_DB5_U8_DCFIX)
    rows = plan.exec_host(raw, FRAMES, flip=True)
    plan.close()
    assert rows.shape == (FRAMES, N)
    down = TR.detect(rows, 0, FRAMES, *DETECTOR)
    across = R.detect(rows, *DETECTOR)
    return str(path), rows, across, down


def expected_events(mask, rows):
    runs = E.runs_of(mask, rows, gap_cols=2)
    events, _ = E.link(runs, 2, 1, 1, 1, 40)
    return runs, events


def tool(name, path, *options):
    r = subprocess.run([os.path.join(BIN, name), path, "--size", str(N), "--flip", "--offset", str(DETECTOR[2])] + list(options),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_the_burst_straddles_the_seam(recording):
    _, rows, across, down = recording
    seam = CHUNK - 18
    assert BURST[0] < seam < BURST[1] - 1
    inside = down[BURST[0]:BURST[1]]
    assert (inside != 0).mean() > 0.3                                                  # the time axis finds the burst (0.45 of its cells)
    assert (across[BURST[0]:BURST[1]] != 0).mean() < 0.05                              # the frequency axis does not
    runs, events = expected_events(down, rows)
    assert any(int(e["row_first"]) < seam <= int(e["row_last"]) and int(e["col_last"]) - int(e["col_first"]) > N // 2 for e in events)


def test_events_tool_down_the_time_axis_and_on_either(recording):
    path, rows, across, down = recording
    for axis, mask in (("time", down), ("either", TR.combine(across, down, TR.MASK_OR))):
        runs, events = expected_events(mask, rows)
        lines = tool("fsea-events", path, "--axis", axis, *EVENT_OPTIONS).split("\n")
        assert lines[0] == "rows %d runs %d events %d" % (FRAMES, runs.size, events.size) and events.size >= 1, axis
        assert lines[1:-1] == event_lines(events) and lines[-1] == "", axis
    assert tool("fsea-events", path, "--axis", "freq", *EVENT_OPTIONS) == tool("fsea-events", path, *EVENT_OPTIONS)
    runs, events = expected_events(across, rows)
    assert tool("fsea-events", path, *EVENT_OPTIONS).split("\n")[0] == "rows %d runs %d events %d" % (FRAMES, runs.size, events.size)
    # --rank stays the frequency detector's under --axis either
    ranked = fsea.OsCfar(N)
    ranked.set(2, 16, DETECTOR[2], 24)
    os_mask = ranked.add(rows, mask=True)
    ranked.close()
    runs, events = expected_events(TR.combine(os_mask, down, TR.MASK_OR), rows)
    lines = tool("fsea-events", path, "--axis", "either", "--rank", "24", *EVENT_OPTIONS).split("\n")
    assert lines[0] == "rows %d runs %d events %d" % (FRAMES, runs.size, events.size) and lines[1:-1] == event_lines(events)


def test_occupancy_tool_down_the_time_axis(recording, tmp_path):
    from PIL import Image
    path, rows, across, down = recording
    out = tmp_path / "mask.png"
    text = tool("fsea-occupancy", path, "--axis", "time", "--min-duty", "0.0005", "--mask", str(out))
    bands = R.bands_of(R.hits_of(down), FRAMES, 0.0005, 0, 1)
    lines = ["%d %d %d %.6f" % (b["first"], b["last"], b["peak"], b["peak_hits"] / FRAMES) for b in bands]
    assert text.split("\n")[0] == "rows %d" % FRAMES and text.split("\n")[1:1 + len(lines)] == lines and len(lines) >= 1
    with Image.open(out) as im:
        assert np.array_equal(np.array(im), down)
    either = TR.combine(across, down, TR.MASK_OR)
    text = tool("fsea-occupancy", path, "--axis", "either", "--min-duty", "0.0005")       # no --mask: the tool keeps one of its own
    bands = R.bands_of(R.hits_of(either), FRAMES, 0.0005, 0, 1)
    lines = ["%d %d %d %.6f" % (b["first"], b["last"], b["peak"], b["peak_hits"] / FRAMES) for b in bands]
    assert text.split("\n")[0] == "rows %d" % FRAMES and text.split("\n")[1:1 + len(lines)] == lines
    assert tool("fsea-occupancy", path, "--axis", "freq") == tool("fsea-occupancy", path)
    # --image: the whole picture through the host form in one call, no context
    Image.fromarray(rows[BURST[0] - 40: BURST[1] + 40]).save(tmp_path / "rows.png")
    part = rows[BURST[0] - 40: BURST[1] + 40]
    r = subprocess.run([os.path.join(BIN, "fsea-occupancy"), "--image", str(tmp_path / "rows.png"), "--offset", str(DETECTOR[2]), "--axis",
                        "time", "--min-duty", "0.05", "--mask", str(out)], capture_output=True, text=True, check=True, timeout=300)
    assert r.stdout.split("\n")[0] == "rows %d" % part.shape[0]
    with Image.open(out) as im:
        assert np.array_equal(np.array(im), TR.detect(part, 0, part.shape[0], *DETECTOR))


def test_cutouts_tool_on_either_axis(recording, tmp_path):
    path, rows, across, down = recording
    runs, events = expected_events(TR.combine(across, down, TR.MASK_OR), rows)
    out = tool("fsea-cutouts", path, "--decimation", "2", "--out", str(tmp_path / "cut"), "--axis", "either", *EVENT_OPTIONS)
    head = out.split()
    assert head[:6] == ["rows", str(FRAMES), "runs", str(runs.size), "events", str(events.size)]
    assert head[6] == "cutouts" and head[8] == "skipped" and int(head[7]) + int(head[9]) == events.size     # the job count
    listed = [line for line in open(tmp_path / "cut" / "cutouts.txt").read().split("\n") if line]
    assert len(listed) == events.size
