"""CPU tier: the argument checks of fsea_persist_*, fsea_cfar_*, fsea_oscfar_* and fsea_events_* that run before any device
work, each with its error code and the whole text of fsea_last_error_string(), against tests/golden/row_messages.json.  The
table was recorded (tests/golden/make_row_messages.py) from the library as it was before the three objects got their shared
checks (csrc/fsea_rows.h), so it pins what a caller saw then: the codes, the texts and, through the cases that break two
rules at once, the order of the checks.  The fsea_oscfar_* entries were recorded from commit 510f74d, which added that
detector as a copy of fsea_cfar's host side: the last one before the two detectors got their shared scaffold
(csrc/fsea_cfar_shared.h).  The substring asserts of test_persist_host.py, test_cfar_host.py, test_oscfar_host.py and
test_events_host.py stay; this is the byte-for-byte layer under them."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from frequensea_amd import fsea

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_messages.json")

P = "P"            # a 16-byte aligned host buffer
OFF = "P+4"        # the same, 4 bytes further on
N = "N"            # a size_t to write a count to
F = "F"            # a fake object of width 64 with no rows so far (the structs begin `int width; int device; uint64_t rows`)
FULL = "FULL"      # the same with 2^32 - 2 rows so far
BIG = (1 << 31) + 1


def _both(name, forms, cases):
    """cases of (label, args) for each (suffix, tail) of `forms`: an entry point's device and host form"""
    return [("%s%s: %s" % (name, suffix, label), name + suffix, tuple(args) + tuple(tail))
            for suffix, tail in forms for label, args in cases]


_ADD = [
    ("NULL object", (None, P, 0, 1, 64)),
    ("type 2", (F, P, 2, 1, 64)),
    ("type -1 before n_rows", (F, P, -1, BIG, 64)),
    ("n_rows above 2^31", (F, P, 0, BIG, 64)),
    ("n_rows above 2^31 before NULL rows", (F, None, 1, BIG, 0)),
    ("no rows", (F, None, 0, 0, 0)),
    ("NULL rows", (F, None, 0, 3, 64)),
    ("NULL rows before pitch", (F, None, 1, 3, 1)),
    ("pitch 63", (F, P, 0, 1, 63)),
    ("pitch 0 of f32 rows", (F, P, 1, 2, 0)),
    ("pitch before span", (F, P, 0, 1 << 31, 63)),
    ("span", (F, P, 0, 4, 1 << 39)),
    ("span of f32 rows", (F, P, 1, 1 << 31, 513)),
    ("rows past 2^32 - 1", (FULL, P, 0, 2, 64)),
    ("no rows for a full object", (FULL, None, 0, 0, 64)),
]
_RUNS = [
    ("NULL object", (None, P, 64, None, 0, 64, 1, None, 0, N)),
    ("NULL n_runs", (F, P, 64, None, 0, 64, 1, None, 0, None)),
    ("NULL n_runs before type", (F, P, 64, None, 5, 64, 1, None, 0, None)),
    ("type 2", (F, P, 64, P, 2, 64, 1, None, 0, N)),
    ("type -1 without levels", (F, P, 64, None, -1, 64, 1, None, 0, N)),
    ("type before n_rows", (F, P, 64, None, 7, 64, BIG, None, 0, N)),
    ("n_rows above 2^31", (F, P, 64, None, 0, 64, BIG, None, 0, N)),
    ("n_rows before capacity", (F, P, 64, None, 0, 64, BIG, None, 3, N)),
    ("capacity without runs", (F, P, 64, None, 0, 64, 1, None, 3, N)),
    ("capacity without runs and no rows", (F, P, 64, None, 0, 64, 0, None, 3, N)),
    ("no rows", (F, None, 0, None, 0, 0, 0, None, 0, N)),
    ("NULL mask", (F, None, 64, None, 0, 64, 2, None, 0, N)),
    ("NULL mask before pitch", (F, None, 1, P, 0, 1, 2, None, 0, N)),
    ("mask pitch 63", (F, P, 63, None, 0, 64, 1, None, 0, N)),
    ("mask pitch before level pitch", (F, P, 0, P, 1, 0, 1, None, 0, N)),
    ("level pitch 63", (F, P, 64, P, 1, 63, 1, None, 0, N)),
    ("level pitch ignored without levels", (F, P, 64, None, 0, 1, 0, None, 0, N)),
    ("level pitch before span", (F, P, 1 << 39, P, 0, 63, 4, None, 0, N)),
    ("mask span", (F, P, 1 << 39, None, 0, 64, 4, None, 0, N)),
    ("level span", (F, P, 64, P, 1, 1 << 39, 4, None, 0, N)),
    ("rows past 2^32 - 1", (FULL, P, 64, None, 0, 64, 2, None, 0, N)),
]
_PAINT = [
    ("NULL object", (None, P, P, 1, 0, 1, P, 64)),
    ("n_rows above 2^31", (F, P, P, 1, 0, BIG, P, 64)),
    ("n_rows before n_runs", (F, P, P, (1 << 32) + 1, 0, BIG, P, 64)),
    ("n_runs above 2^32", (F, P, P, (1 << 32) + 1, 0, 1, P, 64)),
    ("NULL runs", (F, None, P, 1, 0, 1, P, 64)),
    ("NULL values", (F, P, None, 2, 0, 1, P, 64)),
    ("NULL runs and no rows", (F, None, None, 2, 0, 0, P, 64)),
    ("no rows", (F, None, None, 0, 0, 0, None, 0)),
    ("NULL image", (F, P, P, 1, 0, 3, None, 64)),
    ("NULL image before pitch", (F, None, None, 0, 0, 3, None, 1)),
    ("pitch 63", (F, P, P, 1, 0, 1, P, 63)),
    ("pitch before span", (F, P, P, 1, 0, 1 << 31, P, 0)),
    ("span", (F, P, P, 1, 0, 4, P, 1 << 39)),
]
_DEV, _HOST = ("_device", (None,)), ("_host", ())

CASES = (
    # the persistence spectrum
    [("fsea_persist_create: %s" % label, "fsea_persist_create", args) for label, args in (
        ("NULL out", (None, 64, 0)), ("width 0", ("OUT", 0, 0)), ("width above the maximum", ("OUT", (1 << 20) + 1, 0)),
        ("width -1 before the device", ("OUT", -1, 99)))]
    + _both("fsea_persist_add", (_DEV, _HOST), _ADD)
    + [("fsea_persist_add_device: rows off 16 bytes", "fsea_persist_add_device", (F, OFF, 0, 1, 64, None)),
       ("fsea_persist_add_device: pitch before alignment", "fsea_persist_add_device", (F, OFF, 0, 1, 63, None)),
       ("fsea_persist_add_device: alignment before rows past 2^32 - 1", "fsea_persist_add_device", (FULL, OFF, 0, 2, 64, None)),
       ("fsea_persist_add_device: no rows, off 16 bytes", "fsea_persist_add_device", (F, OFF, 0, 0, 64, None)),
       ("fsea_persist_reset: NULL object", "fsea_persist_reset", (None,)),
       ("fsea_persist_destroy: NULL object", "fsea_persist_destroy", (None,)),
       ("fsea_persist_set_range: NULL object", "fsea_persist_set_range", (None, -100.0, 0.0)),
       ("fsea_persist_set_range: lo above hi", "fsea_persist_set_range", (F, 0.0, -100.0)),
       ("fsea_persist_set_range: not finite", "fsea_persist_set_range", (F, float("-inf"), 0.0)),
       ("fsea_persist_set_range: too narrow", "fsea_persist_set_range", (F, 0.0, 1e-45)),
       ("fsea_persist_set_range: fine", "fsea_persist_set_range", (F, -80.0, -20.0)),
       ("fsea_persist_decay: NULL object", "fsea_persist_decay", (None, 1, 2, None)),
       ("fsea_persist_decay: denominator 0", "fsea_persist_decay", (F, 0, 0, None)),
       ("fsea_persist_decay: above one", "fsea_persist_decay", (F, 3, 2, None)),
       ("fsea_persist_decay: one", "fsea_persist_decay", (F, 5, 5, None)),
       ("fsea_persist_counts_host: NULL object", "fsea_persist_counts_host", (None, P)),
       ("fsea_persist_counts_host: NULL counts", "fsea_persist_counts_host", (F, None))]
    + _both("fsea_persist_image", (_DEV, _HOST), [
        ("NULL object", (None, 0, 0, P)), ("map 3", (F, 3, 0, P)), ("map before image", (F, -1, 0, None)),
        ("NULL image", (F, 1, 0, None))])
    + [("fsea_persist_image_device: image off 16 bytes", "fsea_persist_image_device", (F, 0, 0, OFF, None)),
       ("fsea_persist_trace: NULL counts", "fsea_persist_trace", (None, 64, 0, 0.5, P)),
       ("fsea_persist_trace: NULL levels", "fsea_persist_trace", (P, 64, 0, 0.5, None)),
       ("fsea_persist_trace: width 0", "fsea_persist_trace", (P, 0, 0, 0.5, P)),
       ("fsea_persist_trace: kind 3", "fsea_persist_trace", (P, 4, 3, 0.5, P)),
       ("fsea_persist_trace: fraction 1.5", "fsea_persist_trace", (P, 4, 2, 1.5, P)),
       ("fsea_persist_trace: fraction ignored by MAX", "fsea_persist_trace", (P, 4, 0, 1.5, P))]
    # the CFAR detector
    + [("fsea_cfar_create: %s" % label, "fsea_cfar_create", args) for label, args in (
        ("NULL out", (None, 64, 0)), ("width 0", ("OUT", 0, 0)), ("width above the maximum", ("OUT", (1 << 20) + 1, 0)),
        ("width -1 before the device", ("OUT", -1, 99)))]
    + _both("fsea_cfar_add", (("_device", (None, None, None)), ("_host", (None, None))), _ADD)
    + [("fsea_cfar_add_device: rows off 16 bytes", "fsea_cfar_add_device", (F, OFF, 0, 1, 64, None, None, None)),
       ("fsea_cfar_add_device: mask off 16 bytes", "fsea_cfar_add_device", (F, P, 0, 1, 64, OFF, None, None)),
       ("fsea_cfar_add_device: row hits off 16 bytes", "fsea_cfar_add_device", (F, P, 1, 1, 64, P, OFF, None)),
       ("fsea_cfar_add_device: pitch before alignment", "fsea_cfar_add_device", (F, OFF, 0, 1, 63, None, None, None)),
       ("fsea_cfar_add_device: alignment before rows past 2^32 - 1", "fsea_cfar_add_device", (FULL, P, 0, 2, 64, OFF, None, None)),
       ("fsea_cfar_add_device: no rows, off 16 bytes", "fsea_cfar_add_device", (F, OFF, 0, 0, 64, OFF, OFF, None)),
       ("fsea_cfar_reset: NULL object", "fsea_cfar_reset", (None,)),
       ("fsea_cfar_destroy: NULL object", "fsea_cfar_destroy", (None,)),
       ("fsea_cfar_set: NULL object", "fsea_cfar_set", (None, 2, 16, 60, 0)),
       ("fsea_cfar_set: guard -1", "fsea_cfar_set", (F, -1, 16, 60, 0)),
       ("fsea_cfar_set: guard 65 before train", "fsea_cfar_set", (F, 65, 0, 60, 0)),
       ("fsea_cfar_set: train 0", "fsea_cfar_set", (F, 2, 0, 60, 0)),
       ("fsea_cfar_set: train 257", "fsea_cfar_set", (F, 2, 257, 60, 0)),
       ("fsea_cfar_set: offset above", "fsea_cfar_set", (F, 2, 16, (1 << 20) + 1, 0)),
       ("fsea_cfar_set: offset below", "fsea_cfar_set", (F, 2, 16, -(1 << 20) - 1, 0)),
       ("fsea_cfar_set: method 3", "fsea_cfar_set", (F, 2, 16, 60, 3)),
       ("fsea_cfar_set: fine", "fsea_cfar_set", (F, 0, 1, -5, 2)),
       ("fsea_cfar_hits_host: NULL object", "fsea_cfar_hits_host", (None, P)),
       ("fsea_cfar_hits_host: NULL hits", "fsea_cfar_hits_host", (F, None)),
       ("fsea_cfar_bands: NULL hits", "fsea_cfar_bands", (None, 64, 1, 0.5, 0, 1, P, 4, N)),
       ("fsea_cfar_bands: NULL n_bands", "fsea_cfar_bands", (P, 64, 1, 0.5, 0, 1, P, 4, None)),
       ("fsea_cfar_bands: capacity without bands", "fsea_cfar_bands", (P, 64, 1, 0.5, 0, 1, None, 4, N)),
       ("fsea_cfar_bands: width 0", "fsea_cfar_bands", (P, 0, 1, 0.5, 0, 1, P, 4, N)),
       ("fsea_cfar_bands: fraction 1.5", "fsea_cfar_bands", (P, 64, 1, 1.5, 0, 1, P, 4, N)),
       ("fsea_cfar_bands: gap -1", "fsea_cfar_bands", (P, 64, 1, 0.5, -1, 1, P, 4, N)),
       ("fsea_cfar_bands: min_width 0", "fsea_cfar_bands", (P, 64, 1, 0.5, 0, 0, P, 4, N)),
       ("fsea_cfar_bands: no rows", "fsea_cfar_bands", (P, 64, 0, 0.5, 0, 1, None, 0, N))]
    # the ordered-statistic CFAR detector
    + [("fsea_oscfar_create: %s" % label, "fsea_oscfar_create", args) for label, args in (
        ("NULL out", (None, 64, 0)), ("width 0", ("OUT", 0, 0)), ("width above the maximum", ("OUT", (1 << 20) + 1, 0)),
        ("width -1 before the device", ("OUT", -1, 99)))]
    + _both("fsea_oscfar_add", (("_device", (None, None, None)), ("_host", (None, None))), _ADD)
    + [("fsea_oscfar_add_device: rows off 16 bytes", "fsea_oscfar_add_device", (F, OFF, 0, 1, 64, None, None, None)),
       ("fsea_oscfar_add_device: mask off 16 bytes", "fsea_oscfar_add_device", (F, P, 0, 1, 64, OFF, None, None)),
       ("fsea_oscfar_add_device: row hits off 16 bytes", "fsea_oscfar_add_device", (F, P, 1, 1, 64, P, OFF, None)),
       ("fsea_oscfar_add_device: pitch before alignment", "fsea_oscfar_add_device", (F, OFF, 0, 1, 63, None, None, None)),
       ("fsea_oscfar_add_device: alignment before rows past 2^32 - 1", "fsea_oscfar_add_device", (FULL, P, 0, 2, 64, OFF, None, None)),
       ("fsea_oscfar_add_device: no rows, off 16 bytes", "fsea_oscfar_add_device", (F, OFF, 0, 0, 64, OFF, OFF, None)),
       ("fsea_oscfar_reset: NULL object", "fsea_oscfar_reset", (None,)),
       ("fsea_oscfar_destroy: NULL object", "fsea_oscfar_destroy", (None,)),
       ("fsea_oscfar_set: NULL object", "fsea_oscfar_set", (None, 2, 16, 60, 24)),
       ("fsea_oscfar_set: guard -1", "fsea_oscfar_set", (F, -1, 16, 60, 24)),
       ("fsea_oscfar_set: guard 65 before train", "fsea_oscfar_set", (F, 65, 0, 60, 24)),
       ("fsea_oscfar_set: train 0", "fsea_oscfar_set", (F, 2, 0, 60, 24)),
       ("fsea_oscfar_set: train 257", "fsea_oscfar_set", (F, 2, 257, 60, 24)),
       ("fsea_oscfar_set: train 0 before rank", "fsea_oscfar_set", (F, 2, 0, 60, 0)),
       ("fsea_oscfar_set: offset above", "fsea_oscfar_set", (F, 2, 16, (1 << 20) + 1, 24)),
       ("fsea_oscfar_set: offset below", "fsea_oscfar_set", (F, 2, 16, -(1 << 20) - 1, 24)),
       ("fsea_oscfar_set: offset before rank", "fsea_oscfar_set", (F, 2, 16, (1 << 20) + 1, 33)),
       ("fsea_oscfar_set: rank 0", "fsea_oscfar_set", (F, 2, 16, 60, 0)),
       ("fsea_oscfar_set: rank 2 * train + 1", "fsea_oscfar_set", (F, 2, 16, 60, 33)),
       ("fsea_oscfar_set: fine", "fsea_oscfar_set", (F, 0, 1, -5, 2)),
       ("fsea_oscfar_hits_host: NULL object", "fsea_oscfar_hits_host", (None, P)),
       ("fsea_oscfar_hits_host: NULL hits", "fsea_oscfar_hits_host", (F, None))]
    # spectrum events
    + [("fsea_events_create: %s" % label, "fsea_events_create", args) for label, args in (
        ("NULL out", (None, 64, 0)), ("width 0", ("OUT", 0, 0)), ("width above the maximum", ("OUT", (1 << 20) + 1, 0)),
        ("width -1 before the device", ("OUT", -1, 99)))]
    + _both("fsea_events_runs", (_DEV, _HOST), _RUNS)
    + [("fsea_events_runs_device: mask off 16 bytes", "fsea_events_runs_device", (F, OFF, 64, None, 0, 64, 1, None, 0, N, None)),
       ("fsea_events_runs_device: levels off 16 bytes", "fsea_events_runs_device", (F, P, 64, OFF, 1, 64, 1, None, 0, N, None)),
       ("fsea_events_runs_device: runs off 16 bytes", "fsea_events_runs_device", (F, P, 64, None, 0, 64, 1, OFF, 1, N, None)),
       ("fsea_events_runs_device: span before alignment", "fsea_events_runs_device",
        (F, OFF, 1 << 39, None, 0, 64, 4, None, 0, N, None)),
       ("fsea_events_runs_device: alignment before rows past 2^32 - 1", "fsea_events_runs_device",
        (FULL, OFF, 64, None, 0, 64, 2, None, 0, N, None)),
       ("fsea_events_runs_device: no rows, off 16 bytes", "fsea_events_runs_device", (F, OFF, 64, None, 0, 64, 0, None, 0, N, None))]
    + _both("fsea_events_paint", (_DEV, _HOST), _PAINT)
    + [("fsea_events_paint_device: runs off 16 bytes", "fsea_events_paint_device", (F, OFF, P, 1, 0, 1, P, 64, None)),
       ("fsea_events_paint_device: image off 16 bytes", "fsea_events_paint_device", (F, P, P, 1, 0, 1, OFF, 64, None)),
       ("fsea_events_paint_device: pitch before alignment", "fsea_events_paint_device", (F, P, P, 1, 0, 1, OFF, 63, None)),
       ("fsea_events_paint_device: no rows, off 16 bytes", "fsea_events_paint_device", (F, OFF, P, 1, 0, 0, OFF, 64, None)),
       ("fsea_events_reset: NULL object", "fsea_events_reset", (None,)),
       ("fsea_events_destroy: NULL object", "fsea_events_destroy", (None,)),
       ("fsea_events_set_gap: NULL object", "fsea_events_set_gap", (None, 0)),
       ("fsea_events_set_gap: gap -1", "fsea_events_set_gap", (F, -1)),
       ("fsea_events_set_gap: gap 65", "fsea_events_set_gap", (F, 65)),
       ("fsea_events_set_gap: fine", "fsea_events_set_gap", (F, 64)),
       ("fsea_events_link: NULL n_events", "fsea_events_link", (P, 0, 0, 0, 1, 1, 1, None, None, 0, None)),
       ("fsea_events_link: NULL runs", "fsea_events_link", (None, 4, 0, 0, 1, 1, 1, None, None, 0, N)),
       ("fsea_events_link: capacity without events", "fsea_events_link", (None, 0, 0, 0, 1, 1, 1, None, None, 2, N)),
       ("fsea_events_link: n_runs 2^32 - 1", "fsea_events_link", (P, (1 << 32) - 1, 0, 0, 1, 1, 1, None, None, 0, N)),
       ("fsea_events_link: gap_cols -1", "fsea_events_link", (None, 0, -1, 0, 1, 1, 1, None, None, 0, N)),
       ("fsea_events_link: gap_rows above the maximum", "fsea_events_link", (None, 0, 0, (1 << 16) + 1, 1, 1, 1, None, None, 0, N)),
       ("fsea_events_link: min_rows 0", "fsea_events_link", (None, 0, 0, 0, 0, 1, 1, None, None, 0, N)),
       ("fsea_events_link: min_cols 0", "fsea_events_link", (None, 0, 0, 0, 1, 0, 1, None, None, 0, N)),
       ("fsea_events_link: min_hits 0", "fsea_events_link", (None, 0, 0, 0, 1, 1, 0, None, None, 0, N)),
       ("fsea_events_link: no runs", "fsea_events_link", (None, 0, 0, 0, 1, 1, 1, None, None, 0, N))]
)
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def call(case):
    """(code, text): what the case's call returns and, where that is an error, fsea_last_error_string() behind it"""
    _, name, args = case
    L = fsea.hip_lib()
    buf = np.zeros(8192, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    fake = ctypes.create_string_buffer(4096)
    n, out = ctypes.c_size_t(77), ctypes.c_void_p()
    values = {P: p, OFF: p + 4, N: ctypes.byref(n), "OUT": ctypes.byref(out), F: ctypes.cast(fake, ctypes.c_void_p),
              FULL: ctypes.cast(fake, ctypes.c_void_p)}
    struct.pack_into("<iiQ", fake, 0, 64, 0, (1 << 32) - 2 if FULL in args else 0)
    code = getattr(L, name)(*[values[a] if isinstance(a, str) else a for a in args])
    assert not out.value
    return [code, L.fsea_last_error_string().decode() if code else None]


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_is_the_cases(table):
    assert sorted(table) == sorted(IDS)
    # every entry point that takes rows, device and host form, sees each of the shared checks' texts
    for name in ("fsea_persist_add", "fsea_cfar_add", "fsea_oscfar_add", "fsea_events_runs", "fsea_events_paint"):
        for form in ("_device", "_host"):
            texts = " | ".join(t for k, (_, t) in table.items() if k.startswith(name + form + ":") and t)
            for part in ("is NULL", "is more than 2^31", "NULL buffer for the", "is below the width 64", "is too large"):
                assert part in texts, (name + form, part)
            if "paint" not in name:
                assert "type" in texts and "would take rows past 2^32 - 1" in texts, name + form


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_code_and_text(case, table):
    assert call(case) == table[case[0]]
