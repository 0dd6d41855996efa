"""CPU tier: spectrum events without a GPU -- the two numpy restatements of tests/events_ref.py against each other,
fsea_events_link against both and against scipy.ndimage.label, cases one can read off, a list long enough to show a quadratic
sweep, the argument checks of fsea_events_* (before any device work), the header's constants, the tool's usage message and
the shipped kernels' resource usage."""
import ctypes
import os
import re
import struct
import subprocess
import time

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import events_ref as R
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-events")


def random_mask(rng, n, width, density):
    mask = (rng.random((n, width)) < density).astype(np.uint8) * 255
    mask[mask != 0] = rng.choice(np.array([1, 128, 255], np.uint8), int((mask != 0).sum()))    # any byte but 0 is a hit
    return mask


def test_the_two_restatements_agree():
    rng = np.random.default_rng(1)
    cases = 0
    for width in list(range(1, 20)) + [31, 32, 33, 64, 70]:
        for density in (0.05, 0.5, 0.95):
            n = int(rng.integers(1, 13))
            mask = random_mask(rng, n, width, density)
            u8 = rng.integers(0, 256, (n, width), dtype=np.uint8)
            u8[rng.random((n, width)) < 0.5] = 200                                  # ties of the peak
            f32 = rng.normal(-60, 8, (n, width)).astype(np.float32)
            f32[rng.random((n, width)) < 0.1] = np.nan
            for G in (0, 1, 3):
                row0 = int(rng.integers(0, 1000))
                for levels in (None, u8, f32):
                    a, b = R.runs_of(mask, levels, G, row0), R.runs_of_loops(mask, levels, G, row0)
                    assert a.dtype == b.dtype == R.RUN and np.array_equal(a, b), (width, density, G, levels is None)
                runs = R.runs_of(mask, u8, G, row0)
                for gap_rows in (0, 1, 2):
                    filters = [(1, 1, 1), (2, 1, 1), (1, 3, 1), (1, 1, 4), (2, 2, 5)][cases % 5]
                    ea, ra = R.link(runs, G, gap_rows, *filters)
                    eb, rb = R.link_loops(runs, G, gap_rows, *filters)
                    assert np.array_equal(ea, eb) and np.array_equal(ra, rb), (width, density, G, gap_rows, filters)
                    cases += 1
    assert cases > 500


def c_link(runs, gap_cols=0, gap_rows=0, min_rows=1, min_cols=1, min_hits=1, capacity=None):
    """fsea_events_link through ctypes with a capacity of its own: (events written, event_of_run, n_events)."""
    L = fsea.hip_lib()
    runs = np.ascontiguousarray(runs, dtype=fsea.EVENTS_RUN)
    n = ctypes.c_size_t()
    args = (runs.ctypes.data if runs.size else None, runs.size, gap_cols, gap_rows, min_rows, min_cols, min_hits)
    assert L.fsea_events_link(*args, None, None, 0, ctypes.byref(n)) == 0            # capacity 0 with NULL: just counts
    found = n.value
    capacity = found if capacity is None else capacity
    events = np.zeros(capacity + 1, fsea.EVENTS_EVENT)
    events["runs"] = 0xABCD
    of_run = np.full(runs.size, 12345, np.uint32)
    assert L.fsea_events_link(*args, of_run.ctypes.data if runs.size else None, events.ctypes.data, capacity, ctypes.byref(n)) == 0
    assert n.value == found and events["runs"][capacity] == 0xABCD                   # nothing behind the capacity
    return events[:min(capacity, found)], of_run, found


def check_link(runs, *settings):
    want_e, want_r = R.link(runs, *settings)
    got_e, got_r, found = c_link(runs, *settings)
    assert fsea.EVENTS_EVENT == R.EVENT and fsea.EVENTS_RUN == R.RUN and R.EVENT.itemsize == 48 and R.RUN.itemsize == 32
    assert found == want_e.size and np.array_equal(got_e, want_e), (settings, got_e, want_e)
    assert np.array_equal(got_r, want_r), settings
    py_e, py_r = fsea.Events.link(runs, *settings)
    assert np.array_equal(py_e, want_e) and np.array_equal(py_r, want_r)
    return want_e, want_r


def random_runs(rng, n_rows, width, density, G):
    """Runs of a random mask with random levels, the rows spread out and the level sums large."""
    mask = random_mask(rng, n_rows, width, density)
    runs = R.runs_of(mask, rng.integers(0, 256, mask.shape, dtype=np.uint8), G)
    runs["row"] = np.cumsum(rng.integers(1, 4, n_rows))[runs["row"]] + int(rng.integers(0, 1 << 31))
    runs["level_sum"] = rng.integers(-(1 << 62), 1 << 62, runs.size)                 # an event's sum wraps
    return runs


def test_link_against_the_restatement_on_random_run_lists():
    rng = np.random.default_rng(2)
    seen_drop = seen_all = False
    for case in range(150):
        G = int(rng.choice([0, 1, 3, 64]))
        runs = random_runs(rng, int(rng.integers(1, 30)), int(rng.integers(1, 90)), float(rng.choice([0.05, 0.3, 0.7])), G)
        gap_rows = int(rng.integers(0, 4))
        unfiltered, _ = check_link(runs, G, gap_rows)
        if unfiltered.size < 2:
            continue
        hi = unfiltered[unfiltered.size // 2]
        rows_, cols_, hits_ = (int(hi["row_last"] - hi["row_first"] + 1), int(hi["col_last"] - hi["col_first"] + 1), int(hi["hits"]))
        for filters in ((rows_, 1, 1), (1, cols_, 1), (1, 1, hits_), (rows_, cols_, hits_), (1 << 31, 1, 1)):   # each alone, all together
            e, r = check_link(runs, G, gap_rows, *filters)
            seen_drop |= 0 < e.size < unfiltered.size
            assert (r == R.NO_EVENT).any() == (e.size < unfiltered.size)
        seen_all = True
        # a capacity below the number found: the first events in order, the count of all
        got, of_run, found = c_link(runs, G, gap_rows, capacity=unfiltered.size - 1)
        assert found == unfiltered.size and np.array_equal(got, unfiltered[:-1])
    assert seen_drop and seen_all
    e, r = check_link(np.zeros(0, R.RUN))
    assert e.size == 0 and r.size == 0


@pytest.mark.parametrize("density", [0.1, 0.45, 0.8])
def test_link_is_scipys_labelling_at_gap_zero(density):
    """G = gap_rows = 0 without filters is 4-connectivity: the number of events, their boxes and hit counts are those of
    scipy.ndimage.label (default structure) with find_objects."""
    from scipy import ndimage
    mask = random_mask(np.random.default_rng(int(density * 100)), 64, 200, density)
    runs = R.runs_of(mask)
    events, of_run = check_link(runs)
    labels, n = ndimage.label(mask != 0)
    assert events.size == n > 0
    boxes = ndimage.find_objects(labels)
    want = sorted((b[0].start, b[0].stop - 1, b[1].start, b[1].stop - 1, int((labels[b] == k + 1).sum())) for k, b in enumerate(boxes))
    got = sorted((int(e["row_first"]), int(e["row_last"]), int(e["col_first"]), int(e["col_last"]), int(e["hits"])) for e in events)
    assert got == want
    # and the painted labels are scipy's partition
    painted = np.zeros(mask.shape, np.int64)
    for run, k in zip(runs, of_run):
        painted[int(run["row"]), int(run["first"]):int(run["last"]) + 1] = int(k) + 1
    pairs = set(zip(painted[mask != 0].tolist(), labels[mask != 0].tolist()))
    assert len(pairs) == n and not painted[mask == 0].any()


def _mask(rows):
    return np.array([[255 if ch == "#" else 0 for ch in row] for row in rows], np.uint8)


def test_cases_one_can_read_off():
    for gap_rows in (0, 1, 3):
        # two bursts on one column, gap_rows + 2 rows apart: two events; gap_rows + 1 apart: one
        far = np.zeros((gap_rows + 3, 5), np.uint8)
        far[0, 2] = far[gap_rows + 2, 2] = 255
        near = far[1:].copy()
        near[0, 2] = 255
        e, r = check_link(R.runs_of(far), 0, gap_rows)
        assert e.size == 2 and r.tolist() == [0, 1]
        e, r = check_link(R.runs_of(near), 0, gap_rows)
        assert e.size == 1 and r.tolist() == [0, 0]
        assert (int(e[0]["row_first"]), int(e[0]["row_last"]), int(e[0]["runs"]), int(e[0]["hits"])) == (0, gap_rows + 1, 2, 2)
    # an L joins through one shared column; a diagonal pair stays two events; with a column gap of 1 the diagonal touches
    ell = _mask(["#....", "#....", "####."])
    e, _ = check_link(R.runs_of(ell))
    assert e.size == 1 and [int(e[0][k]) for k in ("row_first", "row_last", "col_first", "col_last", "runs", "hits")] == [0, 2, 0, 3, 3, 6]
    diagonal = _mask(["#..", ".#."])
    assert check_link(R.runs_of(diagonal))[0].size == 2
    assert check_link(R.runs_of(diagonal), 1, 0)[0].size == 1
    # touch is first_a <= last_b + G and first_b <= last_a + G: at G = 2 a run ending at 1 reaches one starting at 3, not at 4
    assert check_link(R.runs_of(_mask(["##....", "...#.."])), 2, 0)[0].size == 1
    assert check_link(R.runs_of(_mask(["##....", "....#."])), 2, 0)[0].size == 2
    # two events that a third run joins later keep the position of the first
    e, r = check_link(R.runs_of(_mask(["#...#", "#...#", "#####"])))
    assert e.size == 1 and r.tolist() == [0] * 5
    e, r = check_link(R.runs_of(_mask(["#.#.#", "..#..", "#.#.."])))
    assert r.tolist() == [0, 1, 2, 1, 3, 1] and [int(x) for x in e["col_first"]] == [0, 2, 4, 0]
    # a peak tie goes to the lowest row, then the lowest column
    mask = _mask(["..##.", ".##.."])
    levels = np.array([[0, 0, 7, 9, 0], [0, 9, 9, 0, 0]], np.uint8)
    runs = R.runs_of(mask, levels)
    assert [(int(x["peak"]), int(x["peak_col"]), int(x["level_sum"])) for x in runs] == [(9, 3, 16), (9, 1, 18)]
    e, _ = check_link(runs)
    assert (int(e[0]["peak"]), int(e[0]["peak_row"]), int(e[0]["peak_col"]), int(e[0]["level_sum"])) == (9, 0, 3, 34)
    levels[0, 3] = 8
    e, _ = check_link(R.runs_of(mask, levels))
    assert (int(e[0]["peak"]), int(e[0]["peak_row"]), int(e[0]["peak_col"])) == (9, 1, 1)
    # the filters compare the box and the hits
    e, r = check_link(R.runs_of(_mask(["##..#", "....#"])), 0, 0, 2, 1, 1)
    assert r.tolist() == [R.NO_EVENT, 0, 0] and e.size == 1
    e, r = check_link(R.runs_of(_mask(["##..#", "....#"])), 0, 0, 1, 2, 1)
    assert r.tolist() == [0, R.NO_EVENT, R.NO_EVENT]
    e, r = check_link(R.runs_of(_mask(["##..#", "....#"])), 0, 0, 1, 1, 3)
    assert e.size == 0 and (r == R.NO_EVENT).all()


def test_runs_one_can_read_off():
    mask = _mask(["#.#..#...#"])
    assert [(int(x["first"]), int(x["last"]), int(x["hits"])) for x in R.runs_of(mask)] == [(0, 0, 1), (2, 2, 1), (5, 5, 1), (9, 9, 1)]
    assert [(int(x["first"]), int(x["last"]), int(x["hits"])) for x in R.runs_of(mask, None, 1)] == [(0, 2, 2), (5, 5, 1), (9, 9, 1)]
    assert [(int(x["first"]), int(x["last"]), int(x["hits"])) for x in R.runs_of(mask, None, 2)] == [(0, 5, 3), (9, 9, 1)]
    assert [(int(x["first"]), int(x["last"]), int(x["hits"])) for x in R.runs_of(mask, None, 3, 7)] == [(0, 9, 4)]
    assert R.runs_of(mask, None, 3, 7)["row"].tolist() == [7]
    image = R.paint(R.runs_of(mask, None, 1, 7), [255, 0, 9], 2, 10, row0=6)
    assert image.tolist() == [[0] * 10, [255, 255, 255, 0, 0, 0, 0, 0, 0, 9]]


def test_a_long_list_links_in_linear_time():
    """200 000 runs in 4096 rows: the answer of the restatement's vectorised form.  A sweep that compared every run of a row
    with every run of the rows below would do 10^7 comparisons per gap row here, one over all pairs 2 * 10^10."""
    rng = np.random.default_rng(3)
    n_rows, per_row = 4096, 49
    n = n_rows * per_row
    assert n >= 200000
    first = np.sort(np.argsort(rng.random((n_rows, 2048)), axis=1)[:, :per_row], axis=1) * 4   # distinct multiples of 4 per row
    runs = np.zeros(n, R.RUN)
    runs["row"], runs["first"] = np.repeat(np.arange(n_rows), per_row), first.ravel()
    runs["last"] = runs["first"] + rng.integers(0, 3, n)                                       # below the next multiple: disjoint
    runs["hits"] = runs["last"] - runs["first"] + 1
    runs["peak"] = rng.integers(0, 256, n)
    runs["peak_col"] = runs["first"]
    runs["level_sum"] = runs["peak"]
    want_e, want_r = R.link(runs, 1, 2, 2, 1, 3)
    t0 = time.perf_counter()
    got_e, got_r = fsea.Events.link(runs, 1, 2, 2, 1, 3)
    seconds = time.perf_counter() - t0
    print("linked %d runs into %d events in %.3f s" % (runs.size, got_e.size, seconds))
    assert np.array_equal(got_e, want_e) and np.array_equal(got_r, want_r) and 10 < got_e.size
    assert seconds < 5.0                  # two calls (count, then fetch); a linear sweep takes some tens of milliseconds


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()

    def define(name):
        return eval(re.search(r"#define %s (\(1 << \d+\)|0x[0-9A-Fa-f]+|\d+)" % name, text).group(1))

    assert define("FSEA_EVENTS_MAX_WIDTH") == fsea.EVENTS_MAX_WIDTH == R.MAX_WIDTH == 1 << 20
    assert define("FSEA_EVENTS_MAX_GAP_COLS") == fsea.EVENTS_MAX_GAP_COLS == R.MAX_GAP_COLS == 64
    assert define("FSEA_EVENTS_MAX_GAP_ROWS") == fsea.EVENTS_MAX_GAP_ROWS == R.MAX_GAP_ROWS == 1 << 16
    assert define("FSEA_EVENTS_NO_EVENT") == fsea.EVENTS_NO_EVENT == R.NO_EVENT == 0xFFFFFFFF
    for record, dtype in (("fsea_events_run", fsea.EVENTS_RUN), ("fsea_events_event", fsea.EVENTS_EVENT)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % record, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for ctype, names in re.findall(r"(u?int\d+_t)\s+([^;]+);", body):
            fields += [(name.strip(), {"uint32_t": "<u4", "int32_t": "<i4", "uint64_t": "<u8", "int64_t": "<i8"}[ctype])
                       for name in names.split(",")]
        assert np.dtype(fields) == dtype, record
        offsets = [dtype.fields[name][1] for name, _ in fields]
        assert all(off % np.dtype(kind).itemsize == 0 for off, (_, kind) in zip(offsets, fields))    # C lays it out the same
    assert len([n for n in fsea.EXPORTS if n.startswith("fsea_events_")]) == 11
    assert (fsea.CFAR_U8, fsea.CFAR_F32, fsea.CFAR_F32_SCALE) == (0, 1, 64)                         # the levels are the detector's


def test_events_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    h = ctypes.c_void_p()
    for width in (0, -1, fsea.EVENTS_MAX_WIDTH + 1):
        assert L.fsea_events_create(ctypes.byref(h), width, 0) == FSEA_EINVAL and not h.value, width
        assert b"width" in err()
    assert L.fsea_events_create(None, 64, 0) == FSEA_EINVAL and b"out-pointer" in err()

    buf = np.zeros(8192, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    n = ctypes.c_size_t(77)
    np_ = ctypes.byref(n)
    # a NULL object
    assert L.fsea_events_runs_device(None, p, 64, None, 0, 64, 1, None, 0, np_, None) == FSEA_EINVAL and b"events is NULL" in err()
    assert L.fsea_events_runs_host(None, p, 64, None, 0, 64, 1, None, 0, np_) == FSEA_EINVAL and b"events is NULL" in err()
    assert L.fsea_events_paint_device(None, p, p, 1, 0, 1, p, 64, None) == FSEA_EINVAL and b"events is NULL" in err()
    assert L.fsea_events_paint_host(None, p, p, 1, 0, 1, p, 64) == FSEA_EINVAL and b"events is NULL" in err()
    assert L.fsea_events_reset(None) == FSEA_EINVAL and b"events is NULL" in err()
    assert L.fsea_events_set_gap(None, 0) == FSEA_EINVAL and b"events is NULL" in err()
    assert L.fsea_events_destroy(None) == 0
    assert L.fsea_events_width(None) == 0 and L.fsea_events_rows(None) == 0

    # a fake object: the struct begins with `int width; int device; uint64_t rows; int gap;`; the remaining checks run before
    # anything else of it is used
    fake = ctypes.create_string_buffer(4096)
    struct.pack_into("<iiQi", fake, 0, 64, 0, 0, 0)
    f = ctypes.cast(fake, ctypes.c_void_p)
    assert L.fsea_events_width(f) == 64 and L.fsea_events_rows(f) == 0
    for runs_fn, tail in ((L.fsea_events_runs_device, (None,)), (L.fsea_events_runs_host, ())):
        assert runs_fn(f, p, 64, None, 0, 64, 1, None, 0, None, *tail) == FSEA_EINVAL and b"n_runs is NULL" in err()
        for bad_type in (-1, 2, 7):
            assert runs_fn(f, p, 64, p, bad_type, 64, 1, None, 0, np_, *tail) == FSEA_EINVAL and b"type" in err()
        assert runs_fn(f, p, 64, None, 0, 64, (1 << 31) + 1, None, 0, np_, *tail) == FSEA_EINVAL and b"n_rows" in err()
        assert runs_fn(f, None, 64, None, 0, 64, 1, None, 0, np_, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        assert runs_fn(f, p, 64, None, 0, 64, 1, None, 3, np_, *tail) == FSEA_EINVAL and b"capacity" in err()
        for pitch in (0, 1, 63):
            assert runs_fn(f, p, pitch, None, 0, 64, 1, None, 0, np_, *tail) == FSEA_EINVAL and b"mask pitch" in err()
            assert runs_fn(f, p, 64, p, 1, pitch, 1, None, 0, np_, *tail) == FSEA_EINVAL and b"level pitch" in err()
        assert runs_fn(f, p, 1 << 39, None, 0, 64, 4, None, 0, np_, *tail) == FSEA_EINVAL and b"too large" in err()
        n.value = 77
        assert runs_fn(f, None, 0, None, 0, 0, 0, None, 0, np_, *tail) == 0 and n.value == 0       # n_rows == 0: a no-op
    for off in (1, 4, 8):
        assert L.fsea_events_runs_device(f, p + off, 64, None, 0, 64, 1, None, 0, np_, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_events_runs_device(f, p, 64, p + 1024 + off, 0, 64, 1, None, 0, np_, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_events_runs_device(f, p, 64, None, 0, 64, 1, p + 2048 + off, 1, np_, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_events_paint_device(f, p + off, p, 1, 0, 1, p + 4096, 64, None) == FSEA_EINVAL and b"aligned" in err()
        assert L.fsea_events_paint_device(f, p, p, 1, 0, 1, p + 4096 + off, 64, None) == FSEA_EINVAL and b"aligned" in err()
    # rows would pass 2^32 - 1
    struct.pack_into("<iiQi", fake, 0, 64, 0, (1 << 32) - 2, 0)
    assert L.fsea_events_runs_device(f, p, 64, None, 0, 64, 2, None, 0, np_, None) == FSEA_EINVAL and b"2^32 - 1" in err()
    assert L.fsea_events_runs_host(f, p, 64, None, 0, 64, 2, None, 0, np_) == FSEA_EINVAL and b"2^32 - 1" in err()
    struct.pack_into("<iiQi", fake, 0, 64, 0, 0, 0)
    # the gap
    for gap in (-1, fsea.EVENTS_MAX_GAP_COLS + 1):
        assert L.fsea_events_set_gap(f, gap) == FSEA_EINVAL and b"gap_cols" in err()
    assert L.fsea_events_set_gap(f, fsea.EVENTS_MAX_GAP_COLS) == 0 and struct.unpack_from("<i", fake, 16) == (64,)
    # the paint
    for paint, tail in ((L.fsea_events_paint_device, (None,)), (L.fsea_events_paint_host, ())):
        assert paint(f, None, p, 1, 0, 1, p + 4096, 64, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        assert paint(f, p, None, 1, 0, 1, p + 4096, 64, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        assert paint(f, p, p, 1, 0, 1, None, 64, *tail) == FSEA_EINVAL and b"NULL buffer" in err()
        assert paint(f, p, p, 1, 0, (1 << 31) + 1, p + 4096, 64, *tail) == FSEA_EINVAL and b"n_rows" in err()
        for pitch in (0, 63):
            assert paint(f, p, p, 1, 0, 1, p + 4096, pitch, *tail) == FSEA_EINVAL and b"pitch" in err()
        assert paint(f, None, None, 0, 0, 0, None, 0, *tail) == 0                                  # no rows: a no-op

    # the link: host arithmetic
    runs = R.runs_of(_mask(["#.#", "#.#"]))
    out = np.zeros(4, fsea.EVENTS_EVENT)
    of_run = np.zeros(4, np.uint32)
    rp, op, fp = runs.ctypes.data, out.ctypes.data, of_run.ctypes.data
    assert L.fsea_events_link(rp, 4, 0, 0, 1, 1, 1, fp, op, 4, np_) == 0 and n.value == 2
    assert L.fsea_events_link(rp, 4, 0, 0, 1, 1, 1, None, op, 4, np_) == 0 and n.value == 2      # event_of_run is optional
    assert L.fsea_events_link(None, 4, 0, 0, 1, 1, 1, fp, op, 4, np_) == FSEA_EINVAL and b"NULL" in err()
    assert L.fsea_events_link(rp, 4, 0, 0, 1, 1, 1, fp, op, 4, None) == FSEA_EINVAL and b"NULL" in err()
    assert L.fsea_events_link(rp, 4, 0, 0, 1, 1, 1, fp, None, 4, np_) == FSEA_EINVAL and b"NULL" in err()
    for gap in (-1, fsea.EVENTS_MAX_GAP_COLS + 1):
        assert L.fsea_events_link(rp, 4, gap, 0, 1, 1, 1, fp, op, 4, np_) == FSEA_EINVAL and b"gap_cols" in err()
    for gap in (-1, fsea.EVENTS_MAX_GAP_ROWS + 1):
        assert L.fsea_events_link(rp, 4, 0, gap, 1, 1, 1, fp, op, 4, np_) == FSEA_EINVAL and b"gap_rows" in err()
    assert L.fsea_events_link(rp, 4, 0, fsea.EVENTS_MAX_GAP_ROWS, 1, 1, 1, fp, op, 4, np_) == 0 and n.value == 2
    assert L.fsea_events_link(rp, 4, 0, 0, 0, 1, 1, fp, op, 4, np_) == FSEA_EINVAL and b"min_rows" in err()
    assert L.fsea_events_link(rp, 4, 0, 0, 1, 0, 1, fp, op, 4, np_) == FSEA_EINVAL and b"min_cols" in err()
    assert L.fsea_events_link(rp, 4, 0, 0, 1, 1, 0, fp, op, 4, np_) == FSEA_EINVAL and b"min_hits" in err()


def test_link_refuses_runs_that_are_not_sorted():
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    runs = R.runs_of(_mask(["#.#.", "#..#"]))
    n = ctypes.c_size_t()

    def link(r):
        r = np.ascontiguousarray(r)
        return L.fsea_events_link(r.ctypes.data, r.size, 0, 0, 1, 1, 1, None, None, 0, ctypes.byref(n))

    assert link(runs) == 0 and n.value == 3
    for order in ([1, 0, 2, 3], [2, 3, 0, 1], [0, 1, 3, 2], [0, 0, 1, 2]):                 # within a row, across rows, a repeat
        assert link(runs[order]) == FSEA_EINVAL and b"not sorted" in err(), order
    overlap = runs.copy()
    overlap["last"][0] = 2                                                                # reaches into the next run of its row
    assert link(overlap) == FSEA_EINVAL and b"disjoint" in err()
    backwards = runs.copy()
    backwards["first"][3], backwards["last"][3] = 3, 2
    assert link(backwards) == FSEA_EINVAL and b"above last" in err()
    with pytest.raises(fsea.FseaError, match="not sorted"):
        fsea.Events.link(runs[::-1])


def test_no_gpu_create_says_so():
    if fsea.device_count() > 0:
        pytest.skip("a GPU is present")
    h = ctypes.c_void_p()
    assert fsea.hip_lib().fsea_events_create(ctypes.byref(h), 64, 0) == -2 and not h.value     # FSEA_ENODEVICE
    with pytest.raises(fsea.FseaError, match="no CPU fallback"):
        fsea.Events(64)


def test_tool_usage_message(tmp_path):
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("usage: fsea-events FILE --size N")
    for flag in ("--hop", "--window", "--flip", "--mode db5|db10|db", "--guard", "--train", "--offset LEVELS", "--method ca|go|so",
                 "--gap-cols", "--gap-rows", "--min-rows", "--min-cols", "--min-hits", "--rate HZ --freq MHZ", "--paint OUT.png",
                 "--image IN.png"):
        assert flag in r.stdout, flag
    x = ["x.raw", "--size", "64"]
    for args, text in (([], "no recording file given"), (["x.raw"], "--size"), (["x.raw", "--size", "0"], "--size"),
                       (x + ["--hop", "-1"], "--hop"), (x + ["--method", "os"], "--method"), (x + ["--mode", "db7"], "--mode"),
                       (x + ["--guard", "65"], "--guard"), (x + ["--train", "0"], "--train"), (x + ["--offset", "2000000"], "--offset"),
                       (x + ["--gap-cols", "65"], "--gap-cols"), (x + ["--gap-cols", "-1"], "--gap-cols"),
                       (x + ["--gap-rows", "65537"], "--gap-rows"), (x + ["--min-rows", "0"], "--min-rows"),
                       (x + ["--min-cols", "0"], "--min-cols"), (x + ["--min-hits", "0"], "--min-hits"),
                       (x + ["--rate", "8e6"], "go together"), (x + ["--image", "y.png"], "not both"),
                       (x + ["--bogus"], "usage: fsea-events"), (["--image", str(tmp_path / "missing.png")], "cannot read"),
                       ([str(tmp_path / "missing.raw"), "--size", "64"], "cannot open recording")):
        r = subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and text in r.stderr, (args, r.stderr)


def test_shipped_library_has_the_events_kernels_within_their_budget():
    """The run kernels (pass 1, pass 2 without, with u8 and with f32 levels; 16-byte and element-wise forms), the two scans and
    the paint: wave64, 256 lanes, no scratch, no spilled vector register.  A wave owns a row and keeps its state in registers:
    the only LDS is the scans' four wave sums.  At most 128 VGPRs, so that two workgroups' waves share a SIMD (DESIGN.md
    section 4, "Spectrum events", records the figures)."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    runs = ["fsea_events_count", "fsea_events_runs", "fsea_events_runs_u8", "fsea_events_runs_f32"]
    runs += [name + "_narrow" for name in runs]
    for name in runs + ["fsea_events_scan_rows", "fsea_events_scan_tiles", "fsea_events_paint"]:
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".sgpr_spill_count"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 128, (name, k[".vgpr_count"])
        lds = {"fsea_events_scan_rows": 16, "fsea_events_scan_tiles": 32}.get(name, 0)
        assert k[".group_segment_fixed_size"] == lds, (name, k[".group_segment_fixed_size"])
