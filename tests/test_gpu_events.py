"""GPU tier: spectrum events (fsea_events_*: the run kernels fsea_events_count / fsea_events_runs / _u8 / _f32 and their
element-wise forms, the two scans, fsea_events_paint) and fsea-events.

Every comparison is bit for bit against tests/events_ref.py applied to the very mask and levels given to the object: runs
and images are integers, so there is no tolerance anywhere.  The device forms' outputs are tests/guarded.py payloads of
exactly the documented size (capacity x 32 bytes of records, n_rows x pitch bytes of image): a store outside them dirties a
band.  The inputs are guarded too, fenced with 0xFF in front, behind and between the rows' ends and the pitch: a byte read
from there would be a hit, or a level of 255 (u8) or a NaN (f32)."""
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import cfar_ref as C
from tests import events_ref as R
from tests.conftest import ROOT, synth_iq
from tests.guarded import FILL, Guarded

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "frequensea_amd", "bin")
WIDTHS = [1, 2, 15, 16, 17, 1023, 1024, 1025, 2051]
CHUNK = 1024                                      # cells of a wave's step along its row


def pitches(width):
    """The tight pitch, one that is no multiple of 16 bytes (the element-wise kernels), and whole 16-byte groups with one to
    spare (the 16-byte kernels on rows whose last group is partial)."""
    return width, width + 5, (width + 15) // 16 * 16 + 16


def laid_out(rows, pitch, lead, fence=0xFF):
    """`rows` laid out `pitch` elements apart, `lead` bytes behind the start of a guarded buffer that is otherwise full of
    `fence` bytes.  (the Guarded, the address of row 0)."""
    n, width = rows.shape
    assert lead % 16 == 0 and lead % rows.itemsize == 0
    flat = np.full(lead + max(n, 1) * pitch * rows.itemsize, fence, np.uint8)
    body = flat[lead:].view(rows.dtype)
    for r in range(n):
        body[r * pitch: r * pitch + width] = rows[r]
    g = Guarded(flat.nbytes, fill=fence).upload(flat)
    return g, g.addr + lead


def device_runs(ev, mask, levels=None, G=0, pitch=None, level_pitch=None, lead=0, capacity=None, stream=0):
    """One runs_device at a column gap of G on guarded inputs, into a guarded payload of exactly capacity x 32 bytes (the
    number the restatement finds where capacity is None).  Returns (the records written, the number found)."""
    n, width = mask.shape
    ev.set_gap(G)
    capacity = R.runs_of(mask, None, G).size if capacity is None else capacity
    g_mask, a_mask = laid_out(mask, width if pitch is None else pitch, lead)
    g_lv = a_lv = None
    if levels is not None:
        g_lv, a_lv = laid_out(levels, width if level_pitch is None else level_pitch, lead)
    g_runs = Guarded(capacity * R.RUN.itemsize)
    found = ev.runs_device(a_mask, n, g_runs.addr if capacity else None, capacity, mask_pitch=pitch, d_levels_ptr=a_lv,
                           type=fsea.CFAR_F32 if levels is not None and levels.dtype == np.float32 else fsea.CFAR_U8,
                           level_pitch=level_pitch, stream=stream)
    got = g_runs.payload(R.RUN, (capacity,))
    for g, what in ((g_runs, "runs"), (g_mask, "mask"), (g_lv, "levels")):
        if g is not None:
            g.check(what)
            g.free()
    return got, found


def check(ev, mask, levels=None, G=0, what="", host=True, **kw):
    """Device form (guarded) and host form against the restatement; returns the expected runs (rows from 0)."""
    ev.reset()
    want = R.runs_of(mask, levels, G)
    got, found = device_runs(ev, mask, levels, G, **kw)
    assert found == want.size, (what, found, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "run", int(bad[0]), got[bad[0]], want[bad[0]])
    assert ev.rows == mask.shape[0]
    if host:
        ev.reset()
        assert np.array_equal(ev.runs(mask, levels), want), (what, "host form")
    return want


def random_mask(rng, n, width, density):
    mask = (rng.random((n, width)) < density).astype(np.uint8) * 255
    mask[mask != 0] = rng.choice(np.array([1, 128, 255], np.uint8), int((mask != 0).sum()))    # any byte but 0 is a hit
    return mask


@pytest.mark.parametrize("width", WIDTHS)
def test_random_masks(width):
    """Densities 0.5, 0.01 and 0.99, G 0, 1, 3 and 64, the three pitches, a lead of 32 bytes, with u8 levels, f32 levels and
    none; 65 rows (two workgroups of the scan's neighbours, seventeen of the run kernels), and 1 and 2."""
    rng = np.random.default_rng(width)
    ev = fsea.Events(width)
    assert ev.width == width and ev.rows == 0
    k = 0
    for density in (0.5, 0.01, 0.99):
        mask = random_mask(rng, 65, width, density)
        u8 = rng.integers(0, 256, mask.shape, dtype=np.uint8)
        f32 = rng.uniform(-120, 20, mask.shape).astype(np.float32)
        for G in (0, 1, 3, 64):
            for pitch in pitches(width):
                levels = (None, u8, f32)[(k + k // 3) % 3]               # every kind meets every pitch
                lp = None
                if levels is u8:
                    lp = pitch
                elif levels is f32:
                    lp = (width, width + 3, (width + 3) // 4 * 4 + 4)[k // 9 % 3]
                check(ev, mask, levels, G, what=(width, density, G, pitch, lp), host=pitch == width, pitch=pitch, level_pitch=lp, lead=32)
                k += 1
        for n in (1, 2):
            check(ev, mask[:n], u8[:n], 1, what=(width, density, "rows", n))
    ev.close()


@pytest.mark.parametrize("width", [16, 1024, 1025, 2051, 2064])
def test_masks_one_can_describe(width):
    ev = fsea.Events(width)
    n = 5
    levels = np.random.default_rng(width).integers(0, 256, (n, width), dtype=np.uint8)
    for pitch in pitches(width):
        # all zero: no run, nothing stored
        assert check(ev, np.zeros((n, width), np.uint8), levels, what="zero", pitch=pitch).size == 0
        # all ones: one run per row across every chunk seam
        want = check(ev, np.ones((n, width), np.uint8), levels, what="ones", pitch=pitch)
        assert want.size == n and (want["first"] == 0).all() and (want["last"] == width - 1).all() and (want["hits"] == width).all()
        # a checkerboard: the most runs a row can hold at G = 0, one run at G = 1
        board = ((np.arange(n)[:, None] + np.arange(width)[None, :]) % 2).astype(np.uint8) * 255
        assert check(ev, board, levels, 0, what="board", pitch=pitch).size == board.astype(bool).sum()
        want = check(ev, board, levels, 1, what="board G 1", pitch=pitch)
        assert want.size == n and (want["hits"] == board.astype(bool).sum(axis=1)).all()
    ev.close()


@pytest.mark.parametrize("G", [0, 1, 3, 64])
def test_hits_on_both_sides_of_a_chunk_seam(G):
    """Columns 1023 and 1024 are one run at any G; 1023 and 1024 + G are one run (G free columns between them), 1023 and
    1025 + G are two.  The same one chunk on: 2047 and 2048 + G."""
    width = 2 * CHUNK + 200
    ev = fsea.Events(width)
    levels = np.random.default_rng(G).integers(0, 256, (4, width), dtype=np.uint8)
    mask = np.zeros((4, width), np.uint8)
    mask[0, [CHUNK - 1, CHUNK]] = 255
    mask[1, [CHUNK - 1, CHUNK + G]] = 1
    mask[2, [CHUNK - 1, CHUNK + 1 + G]] = 128
    mask[3, [2 * CHUNK - 1, 2 * CHUNK + G, 2 * CHUNK + 2 * G + 2]] = 255
    for pitch in pitches(width):
        want = check(ev, mask, levels, G, what=("seam", G, pitch), pitch=pitch)
        assert [(int(x["row"]), int(x["first"]), int(x["last"]), int(x["hits"])) for x in want] == [
            (0, CHUNK - 1, CHUNK, 2), (1, CHUNK - 1, CHUNK + G, 2), (2, CHUNK - 1, CHUNK - 1, 1), (2, CHUNK + 1 + G, CHUNK + 1 + G, 1),
            (3, 2 * CHUNK - 1, 2 * CHUNK + G, 2), (3, 2 * CHUNK + 2 * G + 2, 2 * CHUNK + 2 * G + 2, 1)]
    ev.close()


def f32_special_rows(rng, n, width):
    """dB values in [-120, 20], every clamp and NaN, and values whose 64-fold is exactly halfway between two integers."""
    rows = rng.uniform(-120, 20, (n, width)).astype(np.float32)
    half = (np.arange(-40, 40, dtype=np.float32) + np.float32(0.5)) / np.float32(64)
    special = np.concatenate([half, np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 16384.0, -16384.0, 16383.99, -16383.99, 0.0,
                                              -0.0, 3e38, -3e38], np.float32)])
    where = rng.choice(rows.size, size=min(rows.size // 2, 3 * special.size), replace=False)
    rows.ravel()[where] = special[np.arange(where.size) % special.size]
    return rows


@pytest.mark.parametrize("width", [4, 17, 1025, 2051])
def test_levels(width):
    rng = np.random.default_rng(width)
    ev = fsea.Events(width)
    n = 9
    for density in (0.3, 0.9):
        mask = random_mask(rng, n, width, density)
        # u8, the full range; many ties of the peak
        u8 = rng.integers(0, 256, mask.shape, dtype=np.uint8)
        ties = u8.copy()
        ties[rng.random(mask.shape) < 0.6] = 255
        flat = np.full(mask.shape, 7, np.uint8)
        for G in (0, 3):
            for levels in (u8, ties, flat):
                want = check(ev, mask, levels, G, what=(width, density, G, "u8"))
                check(ev, mask, levels, G, what=(width, density, G, "u8 element-wise"), host=False, pitch=width + 5, level_pitch=width + 1, lead=16)
            assert (R.runs_of(mask, flat, G)["peak_col"] == want["first"]).all()            # all equal: the lowest column
        # f32: NaN, the infinities, beyond the clamp, exact halves
        f32 = f32_special_rows(rng, n, width)
        lv = C.levels_of_f32(f32)
        assert width < 1000 or ({-C.LIMIT, C.LIMIT} <= set(lv.ravel().tolist()) and np.isnan(f32).any())
        for G in (0, 1):
            check(ev, mask, f32, G, what=(width, density, G, "f32"))
            check(ev, mask, f32, G, what=(width, density, G, "f32 element-wise"), host=False, pitch=width + 5, level_pitch=width + 3, lead=16)
            check(ev, mask, f32, G, what=(width, density, G, "f32 partial group"), host=False, pitch=(width + 15) // 16 * 16 + 16,
                  level_pitch=(width + 3) // 4 * 4 + 4, lead=32)
        check(ev, mask, None, 1, what=(width, density, "no levels"))
    assert C.levels_of_f32(np.array([0.5 / 64, 1.5 / 64, 2.5 / 64, -0.5 / 64, -1.5 / 64], np.float32)).tolist() == [0, 2, 2, 0, -2]
    ev.close()


def test_a_run_at_the_clamp_whose_sum_passes_2_31():
    """2051 cells at the upper clamp sum to 2051 * 2^20 > 2^31, at the lower clamp to its negative; with one NaN in a run of
    the upper clamp the peak stays 2^20 and the sum drops by 2^21."""
    width = 2051
    ev = fsea.Events(width)
    mask = np.full((3, width), 255, np.uint8)
    levels = np.full((3, width), 1e9, np.float32)
    levels[1] = -1e9
    levels[2, 1500] = np.nan
    for pitch, lp in ((width, width), (width + 5, width + 3), (2064, 2052)):
        want = check(ev, mask, levels, 0, what=("clamp", pitch), pitch=pitch, level_pitch=lp)
        assert want["level_sum"].tolist() == [width << 20, -(width << 20), (width - 2) << 20] and width << 20 > 1 << 31
        assert want["peak"].tolist() == [1 << 20, -(1 << 20), 1 << 20] and want["peak_col"].tolist() == [0, 0, 0]
    ev.close()


def test_capacity():
    """A capacity equal to the number found, one below it (the payload ends where the last record would begin: its 32 bytes
    are the guard band's), far below it, and 0 with NULL."""
    width, n = 1025, 33
    rng = np.random.default_rng(4)
    mask = random_mask(rng, n, width, 0.3)
    levels = rng.integers(0, 256, mask.shape, dtype=np.uint8)
    ev = fsea.Events(width)
    want = R.runs_of(mask, levels, 0)
    assert want.size > 5000
    for capacity in (want.size, want.size - 1, 1000, 1, 0):
        ev.reset()
        got, found = device_runs(ev, mask, levels, capacity=capacity)
        assert found == want.size and np.array_equal(got, want[:capacity]), capacity
    # a capacity above the number found: the rest of the payload is not written
    ev.reset()
    got, found = device_runs(ev, mask, levels, capacity=want.size + 3)
    assert found == want.size and np.array_equal(got[:found], want)
    assert (got[found:].view(np.uint8) == FILL).all()
    # the host form
    ev.reset()
    L = fsea.hip_lib()
    import ctypes
    out = np.zeros(8, R.RUN)
    out["row"] = 99
    k = ctypes.c_size_t()
    assert L.fsea_events_runs_host(ev._p, mask.ctypes.data, width, levels.ctypes.data, 0, width, n, out.ctypes.data, 7, ctypes.byref(k)) == 0
    assert k.value == want.size and np.array_equal(out[:7], want[:7]) and out["row"][7] == 99
    assert L.fsea_events_runs_host(ev._p, mask.ctypes.data, width, None, 0, width, n, None, 0, ctypes.byref(k)) == 0
    assert k.value == want.size and ev.rows == 2 * n
    ev.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_paint(width):
    """Runs from the device list with values 255, 0 and 7; an image of fewer rows than the runs span, so that some fall
    outside; every byte of the n_rows x pitch payload is checked: the image, and the fill between width and pitch."""
    rng = np.random.default_rng(width)
    n = 21
    mask = random_mask(rng, n, width, 0.4 if width > 20 else 0.7)
    ev = fsea.Events(width)
    for G in (0, 3):
        ev.set_gap(G)
        ev.reset()
        want_runs = R.runs_of(mask, None, G)
        g_mask, a_mask = laid_out(mask, width, 0)
        g_runs = Guarded(max(want_runs.size, 1) * R.RUN.itemsize)
        assert ev.runs_device(a_mask, n, g_runs.addr, want_runs.size) == want_runs.size
        values = rng.choice(np.array([255, 0, 7], np.uint8), max(want_runs.size, 1))
        g_values = Guarded(values.size).upload(values)
        for row0, rows in ((0, n), (3, 11), (n + 5, 4)):
            for pitch in pitches(width):
                g_image = Guarded(rows * pitch)
                ev.paint_device(g_runs.addr, g_values.addr, want_runs.size, rows, g_image.addr, row0=row0, pitch=pitch)
                got = g_image.payload(np.uint8, (rows, pitch))
                want = np.full((rows, pitch), FILL, np.uint8)
                want[:, :width] = R.paint(want_runs, values, rows, width, row0)
                assert np.array_equal(got, want), (width, G, row0, pitch, np.argwhere(got != want)[:4].tolist())
                g_image.check("image")
                g_image.free()
            assert np.array_equal(ev.paint(want_runs, values[:want_runs.size], rows, row0), R.paint(want_runs, values, rows, width, row0))
        for g, what in ((g_runs, "runs"), (g_values, "values"), (g_mask, "mask")):
            g.check(what)
            g.free()
    # no run at all: the zero fill alone
    g_image = Guarded(3 * width)
    ev.paint_device(None, None, 0, 3, g_image.addr)
    assert not g_image.payload(np.uint8, (3, width)).any()
    g_image.check("empty image")
    g_image.free()
    ev.close()


def test_paint_reaches_every_alignment():
    """One run per row whose first and last column take every residue modulo 16 against an image base that is aligned: the
    single bytes at both ends and the 16-byte stores between them."""
    width = 200
    runs = np.zeros(16 * 16, R.RUN)
    runs["row"] = np.arange(256)
    runs["first"] = np.arange(256) % 16 + 3
    runs["last"] = runs["first"] + np.arange(256) // 16 * 5 + np.arange(256) % 7
    assert runs["last"].max() < width
    values = (np.arange(256) % 255 + 1).astype(np.uint8)
    ev = fsea.Events(width)
    for pitch in (width, width + 5, 208):
        g_runs, g_values, g_image = Guarded(runs.nbytes).upload(runs), Guarded(256).upload(values), Guarded(256 * pitch)
        ev.paint_device(g_runs.addr, g_values.addr, 256, 256, g_image.addr, pitch=pitch)
        assert np.array_equal(g_image.payload(np.uint8, (256, pitch))[:, :width], R.paint(runs, values, 256, width))
        for g in (g_runs, g_values, g_image):
            g.check("paint")
            g.free()
    ev.close()


def test_the_row_counter_carries_over_calls_and_streams():
    """65 rows given as 1 + 64 give the records of one call; reset brings the counter back; calls on two streams follow one
    another."""
    width, n = 1025, 65
    rng = np.random.default_rng(6)
    mask = random_mask(rng, n, width, 0.05)
    levels = rng.integers(0, 256, mask.shape, dtype=np.uint8)
    ev = fsea.Events(width)
    whole = R.runs_of(mask, levels, 2)
    got, found = device_runs(ev, mask, levels, 2)
    assert found == whole.size and np.array_equal(got, whole) and ev.rows == n
    first, _ = device_runs(ev, mask[:1], levels[:1], 2)                    # rows go on from 65
    rest, _ = device_runs(ev, mask[1:], levels[1:], 2)
    again = np.concatenate([first, rest])
    assert ev.rows == 2 * n and np.array_equal(again["row"], whole["row"] + n)
    again["row"] -= n
    assert np.array_equal(again, whole)
    ev.reset()
    assert ev.rows == 0
    s1, s2 = fsea.Stream(), fsea.Stream()
    a, _ = device_runs(ev, mask[:30], levels[:30], 2, stream=s1)
    b, _ = device_runs(ev, mask[30:], levels[30:], 2, stream=s2)
    assert np.array_equal(np.concatenate([a, b]), whole) and ev.rows == n
    host = np.concatenate([ev.runs(mask[:7], levels[:7]), ev.runs(mask[7:], levels[7:])])
    host["row"] -= n
    assert np.array_equal(host, whole)
    assert ev.runs(mask[:0]).size == 0 and ev.runs_device(0, 0, None, 0) == 0 and ev.rows == 2 * n   # no rows: a no-op
    for o in (s1, s2, ev):
        o.close()
    for _ in range(20):                                                 # create / destroy cycles
        ev = fsea.Events(64)
        ev.runs(mask[:2, :64])
        ev.close()


N, FRAMES = 256, 96
BURSTS = ((16, 32, 40), (56, 80, -70))            # first frame, the frame behind the last, the tone's bin from the centre
DETECTOR = (2, 16, 40, C.CA)
MIN_HITS = 6


def two_bursts():
    """synth_iq's noise (sigma 20, no tone) with two tone bursts of amplitude 40 added: frames 16 .. 31 at bin +40 and frames
    56 .. 79 at bin -70 of 256, whole frames of a whole number of cycles, so each burst is one column: 128 + 40 and
    128 - 70.  With the CPU oracle's DB5 rows, (2, 16, 40, CA) finds 283 runs in 243 events, the bursts with 16 and 24 hits and
    no other event with more than 3; min_hits 6 leaves exactly the two."""
    raw = synth_iq(21, 2 * N * FRAMES, amp=0.0)
    x = raw.view(np.int8).astype(np.float64)
    for f0, f1, k in BURSTS:
        t = np.arange(f0 * N, f1 * N)
        tone = 40.0 * np.exp(2j * np.pi * (k / N) * t)
        x[2 * t] += tone.real
        x[2 * t + 1] += tone.imag
    return np.clip(np.rint(x), -128, 127).astype(np.int8).view(np.uint8)


def boxes(events):
    return [tuple(int(e[k]) for k in ("row_first", "row_last", "col_first", "col_last", "hits")) for e in events]


WANT_BOXES = [(16, 31, 168, 168, 16), (56, 79, 58, 58, 24)]


def test_two_bursts_end_to_end():
    """Plan -> Cfar with a mask -> Events, nothing visits the host in between; the result is the restatement's on the same
    mask and rows, and exactly the two bursts with the boxes of the injection."""
    raw = two_bursts()
    plan = fsea.Plan(N, N, fsea.MODE_DB5_U8_DCFIX)
    d_iq = fsea.DeviceBuffer(raw.nbytes).upload(raw)
    d_rows = fsea.DeviceBuffer(FRAMES * N)
    plan.exec_device(d_iq.ptr.value, FRAMES, d_rows.ptr.value, flip=True)
    cfar = fsea.Cfar(N)
    cfar.set(*DETECTOR)
    g_mask = Guarded(FRAMES * N)
    cfar.add_device(d_rows.ptr.value, fsea.CFAR_U8, FRAMES, N, g_mask.addr)
    ev = fsea.Events(N)
    found = ev.runs_device(g_mask.addr, FRAMES, None, 0)
    g_runs = Guarded(found * R.RUN.itemsize)
    ev.reset()
    assert ev.runs_device(g_mask.addr, FRAMES, g_runs.addr, found, d_levels_ptr=d_rows.ptr.value, type=fsea.CFAR_U8) == found
    rows, mask = d_rows.download(np.uint8, (FRAMES, N)), g_mask.payload(np.uint8, (FRAMES, N))
    runs = g_runs.payload(R.RUN, (found,))
    assert np.array_equal(mask, C.detect(rows, *DETECTOR)) and np.array_equal(runs, R.runs_of(mask, rows))
    events, of_run = fsea.Events.link(runs, 0, 0, 1, 1, MIN_HITS)
    want_e, want_r = R.link(runs, 0, 0, 1, 1, MIN_HITS)
    assert np.array_equal(events, want_e) and np.array_equal(of_run, want_r)
    print("runs %d, events without a filter %d, with min_hits %d: %s" % (found, fsea.Events.link(runs)[0].size, MIN_HITS, boxes(events)))
    assert boxes(events) == WANT_BOXES and found > 100
    assert [(int(e["peak_col"]), int(e["peak"]) > 140) for e in events] == [(168, True), (58, True)]
    # the cleaned mask: the two bursts alone
    values = np.where(of_run != R.NO_EVENT, 255, 0).astype(np.uint8)
    g_values, g_image = Guarded(values.size).upload(values), Guarded(FRAMES * N)
    ev.paint_device(g_runs.addr, g_values.addr, found, FRAMES, g_image.addr)
    clean = g_image.payload(np.uint8, (FRAMES, N))
    want = np.zeros((FRAMES, N), np.uint8)
    for (f0, f1, k) in BURSTS:
        want[f0:f1, N // 2 + k] = 255
    assert np.array_equal(clean, want)
    for g in (g_mask, g_runs, g_values, g_image):
        g.check("end to end")
        g.free()
    for o in (ev, cfar, plan):
        o.close()
    d_iq.free()
    d_rows.free()


def python_path(rows, gap_cols, gap_rows, min_rows, min_cols, min_hits, detector):
    """What the tool does, through the binding: (runs, events, the painted image)."""
    cfar, ev = fsea.Cfar(rows.shape[1]), fsea.Events(rows.shape[1])
    cfar.set(*detector)
    mask = cfar.add(rows, mask=True)
    ev.set_gap(gap_cols)
    runs = ev.runs(mask, rows)
    events, of_run = fsea.Events.link(runs, gap_cols, gap_rows, min_rows, min_cols, min_hits)
    image = ev.paint(runs, np.where(of_run != R.NO_EVENT, 255, 0).astype(np.uint8), rows.shape[0])
    cfar.close()
    ev.close()
    return runs, events, image


def event_lines(events, mhz=None, seconds=None):
    lines = []
    for e in events:
        line = "%d %d %d %d %d %d %d %d" % tuple(int(e[k]) for k in ("row_first", "row_last", "col_first", "col_last", "hits", "peak",
                                                                     "peak_row", "peak_col"))
        if mhz:
            line += "".join(" %.6f" % mhz(int(e[k])) for k in ("col_first", "col_last", "peak_col"))
        if seconds:
            line += "".join(" %.6f" % seconds(int(e[k])) for k in ("row_first", "row_last", "peak_row"))
        lines.append(line)
    return lines


def test_tool_on_a_recording_and_on_an_image(tmp_path):
    from PIL import Image
    raw = two_bursts()
    tail = synth_iq(5, 100, amp=0.0)                                   # 50 samples over: no further frame
    np.concatenate([raw, tail]).tofile(tmp_path / "bursts.raw")
    plan = fsea.Plan(N, N, fsea.MODE_DB5_U8_DCFIX)
    rows = plan.exec_host(raw, FRAMES, flip=True)
    plan.close()
    tool = os.path.join(BIN, "fsea-events")
    rate, freq = 8000000.0, 100.0
    # the two bursts alone, with MHz and seconds
    out = tmp_path / "clean.png"
    r = subprocess.run([tool, str(tmp_path / "bursts.raw"), "--size", str(N), "--flip", "--offset", "40", "--min-hits", str(MIN_HITS),
                        "--rate", "8000000", "--freq", "100", "--paint", str(out)], capture_output=True, text=True, check=True, timeout=300)
    runs, events, image = python_path(rows, 0, 0, 1, 1, MIN_HITS, DETECTOR)
    assert boxes(events) == WANT_BOXES
    lines = r.stdout.split("\n")
    assert lines[0] == "rows %d runs %d events 2" % (FRAMES, runs.size)
    assert lines[1:3] == event_lines(events, lambda k: freq + (k - N // 2) * rate / N / 1e6, lambda row: row * N / rate)
    assert lines[3:] == ["Written %s." % out, ""]                      # the PNG writer's own line
    assert lines[1].split()[8:] == ["101.250000", "101.250000", "101.250000", "0.000512", "0.000992"] + ["%.6f" % (int(events[0]["peak_row"]) * N / rate)]
    with Image.open(out) as im:
        got = np.array(im)
    assert got.dtype == np.uint8 and np.array_equal(got, image) and (got != 0).sum() == 40
    # every event, joined across gaps: another detector setting, gaps and filters; no --rate: the eight numbers alone
    settings = (3, 2, 2, 1, 3)
    r = subprocess.run([tool, str(tmp_path / "bursts.raw"), "--size", str(N), "--flip", "--guard", "1", "--train", "12", "--offset", "35",
                        "--method", "so", "--gap-cols", "3", "--gap-rows", "2", "--min-rows", "2", "--min-cols", "1", "--min-hits", "3",
                        "--paint", str(out)], capture_output=True, text=True, check=True, timeout=300)
    runs, events, image = python_path(rows, *settings, (1, 12, 35, C.SO))
    lines = r.stdout.split("\n")
    assert lines[0] == "rows %d runs %d events %d" % (FRAMES, runs.size, events.size) and events.size > 2
    assert lines[1:-2] == event_lines(events) and lines[-2].startswith("Written ")
    with Image.open(out) as im:
        assert np.array_equal(np.array(im), image)
    # the same rows as a small 8-bit grey image: the same events, MHz without seconds
    Image.fromarray(rows[:40]).save(tmp_path / "rows.png")
    r = subprocess.run([tool, "--image", str(tmp_path / "rows.png"), "--offset", "40", "--gap-cols", "1", "--min-hits", "2", "--rate",
                        "8000000", "--freq", "100", "--paint", str(out)], capture_output=True, text=True, check=True, timeout=300)
    runs, events, image = python_path(rows[:40], 1, 0, 1, 1, 2, DETECTOR)
    lines = r.stdout.split("\n")
    assert lines[0] == "rows 40 runs %d events %d" % (runs.size, events.size) and events.size >= 1
    assert lines[1:-2] == event_lines(events, lambda k: freq + (k - N // 2) * rate / N / 1e6) and lines[-2].startswith("Written ")
    with Image.open(out) as im:
        assert np.array_equal(np.array(im), image)
