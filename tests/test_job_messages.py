"""CPU tier: the argument checks of fsea_extract_* and fsea_measure_* that run before any device work, each with its error
code and the whole text of fsea_last_error_string(), against tests/golden/job_messages.json.  The table was recorded
(tests/golden/make_job_messages.py) from the library as it was before the two objects got their shared checks
(csrc/fsea_jobs.h), so it pins what a caller saw then: the codes, the texts and, through the cases that break two rules at
once, the order of the checks.  The argument sets are those of test_extract_host.py and test_measure_host.py, whose
substring asserts stay; this is the byte-for-byte layer under them."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from frequensea_amd import fsea

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "job_messages.json")

P, P4, P1 = "P", "P+4", "P+1"          # a 16-byte aligned host buffer: the input of a run
S, S8 = "S", "S+8"                     # the same 4096 bytes further on: the output of a run
N = "N"                                # a size_t to write a count to
EV, FT = "EV", "FT"                    # two zeroed events, two bytes for their fits
FM = "FM"                              # a fake fsea_measure: zeroes, the checks read nothing of it
MAX = 65536                            # FSEA_EXTRACT_MAX_JOBS and FSEA_MEASURE_MAX_JOBS
BIG = 1 << 40
NAN, INF = float("nan"), float("inf")


def X(d):
    """a fake fsea_extract of 97 taps and decimation d: the struct begins `int n_taps; int decimation; int device`"""
    return ("X", d)


def E(*jobs):
    """a table of fsea_extract_job"""
    return ("E", jobs)


def M(*jobs):
    """a table of fsea_measure_job (first_pair, n_pairs)"""
    return ("M", jobs)


def job(first=0, n=64, offset=0, cps=0.01, phase0=0.0, out_first=0):
    return (first, n, offset, cps, phase0, out_first)


ONE = E(job())

# fsea_extract_run_*(x, iq, n_iq, flip, jobs, n_jobs, pairs, capacity[, stream])
_EXTRACT_RUN = [
    ("NULL object", (None, None, 0, 0, None, MAX + 1, None, 0)),
    ("n_jobs above the maximum", (X(4), None, 0, 0, None, MAX + 1, None, 0)),
    ("no jobs", (X(4), None, 0, 0, None, 0, None, 0)),
    ("no jobs, whatever else", (X(4), P4, 7, 1, None, 0, S8, 0)),
    ("NULL job table", (X(4), None, 512, 0, None, 1, None, 512)),
    ("NULL input", (X(4), None, 512, 0, ONE, 1, S, 512)),
    ("NULL output", (X(4), P, 512, 0, ONE, 1, None, 512)),
] + [(label, (X(d), P, n_iq, 0, E(*jobs), len(jobs), S, capacity)) for label, jobs, n_iq, capacity, d in (
    ("job 1 past the input", [job(), job(first=500, n=13)], 512, 512, 4),
    ("first past the input", [job(first=BIG)], 512, 512, 4),
    ("first + n wraps", [job(n=(1 << 64) - 1, first=2)], 512, 512, 4),
    ("n_samples too large", [job(n=(1 << 31) + 1)], BIG, 512, 4),
    ("past the input before too large", [job(n=(1 << 31) + 1, first=BIG)], BIG, 512, 4),
    ("cycles_per_sample nan", [job(), job(cps=NAN)], 512, 512, 4),
    ("cycles_per_sample inf", [job(), job(cps=INF)], 512, 512, 4),
    ("cycles_per_sample 2^21", [job(), job(cps=2.0 ** 21)], 512, 512, 4),
    ("phase0 nan", [job(phase0=NAN)], 512, 512, 4),
    ("phase0 -inf", [job(phase0=-INF)], 512, 512, 4),
    ("sample_offset above 2^52", [job(offset=(1 << 52) + 1)], 512, 512, 4),
    ("sample_offset + n_samples above 2^52", [job(offset=(1 << 52) - 63)], 512, 512, 4),
    ("table order", [job(n=1 << 31, cps=NAN), job(n=(1 << 31) + 1)], BIG, 512, 4),
    ("the total", [job(n=1 << 31)] * 4 + [job(n=4)], BIG, BIG, 4),
    ("jobs before the total", [job(n=1 << 31), job(n=1, cps=INF)], BIG, BIG, 1),
    ("the total before the ranges", [job(n=1 << 31, out_first=1 << 33), job(n=1)], BIG, 4, 1),
    ("outputs one past the capacity", [job(out_first=497)], 512, 512, 4),
    ("out_first past the capacity", [job(out_first=BIG)], 512, 512, 4),
    ("out_first + outputs wraps", [job(), job(out_first=(1 << 64) - 1)], 512, 512, 4),
    ("jobs 0 and 2 overlap", [job(out_first=40), job(n=3, out_first=44), job(out_first=30), job(out_first=45)], 512, 512, 4),
    ("jobs 0 and 1 overlap", [job(out_first=8), job(out_first=8)], 512, 512, 4),
    ("capacity before overlap", [job(out_first=600), job(out_first=0), job(out_first=15)], 512, 512, 4),
)]
# jobs without output take no room, anywhere, also on top of another: this table passes every check but the alignment
_EMPTY = E(job(out_first=0), job(n=3, out_first=5), job(n=0, out_first=1 << 50))
_OVER = E(job(out_first=8), job(out_first=8))

# fsea_measure_run_*(m, pairs, n_buffer, jobs, n_jobs, offset_re, offset_im, lag, sums[, stream])
_M1 = M((0, 64))
_MEASURE_RUN = [
    ("NULL object", (None, None, 512, None, MAX + 1, 0.5, 0.5, 0, S)),
    ("n_jobs above the maximum", (FM, None, 512, None, MAX + 1, 0.5, 0.5, 0, S)),
    ("no jobs", (FM, None, 0, None, 0, NAN, 0.0, 0, None)),
    ("no jobs, whatever else", (FM, P4, 7, None, 0, 0.0, 0.0, 1, S8)),
    ("NULL job table", (FM, None, 512, None, 1, 0.5, 0.5, 0, S)),
    ("NULL input before lag", (FM, None, 512, _M1, 1, 0.5, 0.5, 0, S)),
    ("NULL output before lag", (FM, P, 512, _M1, 1, 0.5, 0.5, 0, None)),
    ("lag 0 before offset", (FM, P, 512, _M1, 1, NAN, 0.0, 0, S)),
    ("lag -3 before offset", (FM, P, 512, _M1, 1, NAN, 0.0, -3, S)),
    ("lag above the maximum", (FM, P, 512, _M1, 1, NAN, 0.0, 65537, S)),
    ("offset nan before jobs", (FM, P, 512, M((600, 1)), 1, NAN, 0.0, 1, S)),
    ("offset inf", (FM, P, 512, M((600, 1)), 1, 0.0, INF, 1, S)),
    ("offset -inf", (FM, P, 512, M((600, 1)), 1, -INF, 0.0, 1, S)),
    ("job 1 past the buffer", (FM, P, 512, M((0, 64), (500, 13)), 2, 0.5, 0.5, 1, S)),
    ("first past the buffer", (FM, P, 512, M((BIG, 1)), 1, 0.5, 0.5, 1, S)),
    ("first + n wraps", (FM, P, 512, M((2, (1 << 64) - 1)), 1, 0.5, 0.5, 1, S)),
    ("n_pairs too large", (FM, P, BIG, M((0, (1 << 24) + 1)), 1, 0.5, 0.5, 1, S)),
    ("job 1 past a large buffer", (FM, P, BIG, M((0, 1 << 24), (BIG, 1)), 2, 0.5, 0.5, 1, S)),
    ("the total before alignment", (FM, P4, BIG, M(*[(0, 1 << 24)] * 129), 129, 0.5, 0.5, 1, S)),
    ("a job before the total", (FM, P, BIG, M(*([(0, 1 << 24)] * 129 + [(BIG, 1)])), 130, 0.5, 0.5, 1, S)),
]
_DEV, _HOST = ("_device", (None,)), ("_host", ())


def _both(name, cases):
    return [("%s%s: %s" % (name, suffix, label), name + suffix, tuple(args) + tail) for suffix, tail in (_DEV, _HOST) for label, args in cases]


_EJ = (EV, 2, 1024, 1024, 1 << 20, 97, 16, 0.8, E(job(), job()), FT)       # fsea_extract_jobs, all fine


def _ej(**changed):
    names = ("events", "n_events", "width", "hop", "n_samples", "n_taps", "decimation", "max_fill", "jobs", "fits")
    return tuple(changed.get(k, v) for k, v in zip(names, _EJ))


_TWO = E(job(first=0, n=64, offset=0, cps=0.0, out_first=0), job(first=0, n=(1 << 24) + 8, offset=0, cps=0.0, out_first=0))
_OUT2 = M((0, 0), (0, 0))

CASES = (
    _both("fsea_extract_run", _EXTRACT_RUN)
    + [("fsea_extract_run_device: alignment behind the jobs' checks", "fsea_extract_run_device", (X(4), P4, 512, 0, _EMPTY, 3, S, 512, None)),
       ("fsea_extract_run_device: input off 16 bytes", "fsea_extract_run_device", (X(4), P4, 512, 0, ONE, 1, S, 512, None)),
       ("fsea_extract_run_device: output off 16 bytes", "fsea_extract_run_device", (X(4), P, 512, 0, ONE, 1, S8, 512, None)),
       ("fsea_extract_run_device: input off 1 byte", "fsea_extract_run_device", (X(4), P1, 512, 0, ONE, 1, S, 512, None)),
       ("fsea_extract_run_device: overlap before alignment", "fsea_extract_run_device", (X(4), P4, 512, 0, _OVER, 2, S, 512, None)),
       ("fsea_extract_layout: NULL object", "fsea_extract_layout", (None, ONE, 1, N)),
       ("fsea_extract_layout: NULL total_pairs", "fsea_extract_layout", (X(4), ONE, 1, None)),
       ("fsea_extract_layout: NULL job table", "fsea_extract_layout", (X(4), None, 1, N)),
       ("fsea_extract_layout: n_jobs above the maximum", "fsea_extract_layout", (X(4), ONE, MAX + 1, N)),
       ("fsea_extract_layout: total_pairs before n_jobs", "fsea_extract_layout", (X(4), None, MAX + 1, None)),
       ("fsea_extract_layout: no jobs", "fsea_extract_layout", (X(4), None, 0, N)),
       ("fsea_extract_jobs: fine", "fsea_extract_jobs", _EJ),
       ("fsea_extract_jobs: NULL events", "fsea_extract_jobs", _ej(events=None)),
       ("fsea_extract_jobs: NULL jobs", "fsea_extract_jobs", _ej(jobs=None)),
       ("fsea_extract_jobs: NULL fits", "fsea_extract_jobs", _ej(fits=None)),
       ("fsea_extract_jobs: no events", "fsea_extract_jobs", _ej(events=None, n_events=0, jobs=None, fits=None)),
       ("fsea_extract_jobs: width 0", "fsea_extract_jobs", _ej(width=0)),
       ("fsea_extract_jobs: width -4", "fsea_extract_jobs", _ej(width=-4)),
       ("fsea_extract_jobs: hop 0", "fsea_extract_jobs", _ej(hop=0)),
       ("fsea_extract_jobs: hop -1", "fsea_extract_jobs", _ej(hop=-1)),
       ("fsea_extract_jobs: n_taps 0", "fsea_extract_jobs", _ej(n_taps=0)),
       ("fsea_extract_jobs: n_taps 513", "fsea_extract_jobs", _ej(n_taps=513)),
       ("fsea_extract_jobs: decimation 0", "fsea_extract_jobs", _ej(decimation=0)),
       ("fsea_extract_jobs: decimation 65", "fsea_extract_jobs", _ej(decimation=65)),
       ("fsea_extract_jobs: max_fill 0", "fsea_extract_jobs", _ej(max_fill=0.0)),
       ("fsea_extract_jobs: max_fill -0.5", "fsea_extract_jobs", _ej(max_fill=-0.5)),
       ("fsea_extract_jobs: max_fill above 1", "fsea_extract_jobs", _ej(max_fill=1.0000001)),
       ("fsea_extract_jobs: max_fill nan", "fsea_extract_jobs", _ej(max_fill=NAN)),
       ("fsea_extract_jobs: max_fill inf", "fsea_extract_jobs", _ej(max_fill=INF)),
       ("fsea_extract_jobs: max_fill 1", "fsea_extract_jobs", _ej(max_fill=1.0)),
       ("fsea_extract_jobs: width before hop", "fsea_extract_jobs", _ej(width=0, hop=0, n_taps=0))]
    + _both("fsea_measure_run", _MEASURE_RUN)
    + [("fsea_measure_run_device: input off 8 bytes", "fsea_measure_run_device", (FM, P4, 512, _M1, 1, 0.5, 0.5, 1, S, None)),
       ("fsea_measure_run_device: output off 16 bytes", "fsea_measure_run_device", (FM, P, 512, _M1, 1, 0.5, 0.5, 1, S8, None)),
       ("fsea_measure_run_device: input off 1 byte", "fsea_measure_run_device", (FM, P1, 512, _M1, 1, 0.5, 0.5, 1, S, None)),
       ("fsea_measure_jobs: too many pairs", "fsea_measure_jobs", (_TWO, 2, 1, 7, _OUT2)),
       ("fsea_measure_jobs: fine", "fsea_measure_jobs", (_TWO, 2, 1, 8, _OUT2)),
       ("fsea_measure_jobs: decimation 0", "fsea_measure_jobs", (_TWO, 2, 0, 0, _OUT2)),
       ("fsea_measure_jobs: NULL extract jobs", "fsea_measure_jobs", (None, 2, 1, 0, _OUT2)),
       ("fsea_measure_jobs: NULL jobs", "fsea_measure_jobs", (_TWO, 2, 1, 0, None)),
       ("fsea_measure_jobs: n_jobs above the maximum", "fsea_measure_jobs", (_TWO, MAX + 1, 1, 0, _OUT2)),
       ("fsea_measure_jobs: n_jobs before the tables", "fsea_measure_jobs", (None, MAX + 1, 0, 0, None)),
       ("fsea_measure_jobs: no jobs", "fsea_measure_jobs", (None, 0, 1, 0, None))]
)
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def call(case):
    """(code, text): what the case's call returns and, where that is an error, fsea_last_error_string() behind it"""
    _, name, args = case
    L = fsea.hip_lib()
    buf = np.full(8192 + 16, 0x5A, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    n = ctypes.c_size_t(77)
    events, fits = np.zeros(2, fsea.EVENTS_EVENT), np.zeros(2, np.uint8)
    values = {P: p, P4: p + 4, P1: p + 1, S: p + 4096, S8: p + 4096 + 8, N: ctypes.byref(n), EV: events.ctypes.data, FT: fits.ctypes.data,
              FM: ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)}
    alive = []

    def value(a):
        if isinstance(a, str):
            return values[a]
        if not isinstance(a, tuple):
            return a
        if a[0] == "X":
            fake = ctypes.create_string_buffer(4096)
            struct.pack_into("<iii", fake, 0, 97, a[1], 0)
            alive.append(fake)
            return ctypes.cast(fake, ctypes.c_void_p)
        kind = fsea.ExtractJob if a[0] == "E" else fsea.MeasureJob
        alive.append((kind * len(a[1]))(*[kind(*j) for j in a[1]]))
        return ctypes.addressof(alive[-1])

    code = getattr(L, name)(*[value(a) for a in args])
    assert np.all(buf == 0x5A)                 # a refused call writes nothing, nor does one without jobs
    return [code, L.fsea_last_error_string().decode() if code else None]


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_is_the_cases(table):
    assert sorted(table) == sorted(IDS)
    # both objects, device and host form, see each of the shared checks' texts with their own nouns
    shared = ("is NULL", "n_jobs 65537 above 65536", "NULL job table", "NULL buffer", "lie past the", "too large", "more than 2^31")
    for name, nouns in (("fsea_extract_run", ("samples", "of the input", "outputs in one call")),
                        ("fsea_measure_run", ("pairs", "of the buffer", "pairs in one call"))):
        for form in ("_device", "_host"):
            texts = " | ".join(t for k, (_, t) in table.items() if k.startswith(name + form + ":") and t)
            for part in shared + nouns:
                assert part in texts, (name + form, part)
            assert [table["%s%s: %s" % (name, form, k)] for k in ("no jobs", "no jobs, whatever else")] == [[0, None], [0, None]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_code_and_text(case, table):
    assert call(case) == table[case[0]]
