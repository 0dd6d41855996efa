"""CPU tier: the argument checks of fsea_extract_*, fsea_measure_* and fsea_audio_* that run before any device work, each
with its error code and the whole text of fsea_last_error_string(), against tests/golden/job_messages.json.  The table was
recorded (tests/golden/make_job_messages.py) from the library as it was before the objects' checks were shared
(csrc/fsea_jobs.h) -- extract's and measure's before the two got theirs, audio's before its placement check, table build and
host form joined them -- so it pins what a caller saw then: the codes, the texts and, through the cases that break two rules
at once, the order of the checks.  The argument sets are those of test_extract_host.py, test_measure_host.py and
test_audio_host.py, whose substring asserts stay; this is the byte-for-byte layer under them."""
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
S2, S1 = "S+2", "S+1"
N = "N"                                # a size_t to write a count to
EV, FT = "EV", "FT"                    # two zeroed events, two bytes for their fits
FM = "FM"                              # a fake fsea_measure: zeroes, the checks read nothing of it
H = "H"                                # a handle to write a new object to
T, TB = "T", "TB"                      # 21 taps of 1.0; the same with a NaN as tap 3
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


def FA(d):
    """a fake fsea_audio (FM, 41 taps) of decimation d: the struct begins `int kind; int n_taps; int decimation; int device`"""
    return ("A", d)


def AJ(*jobs):
    """a table of fsea_audio_job (first_pair, n_pairs, out_first)"""
    return ("AJ", jobs)


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

# fsea_audio_run_*(a, pairs, n_buffer, jobs, n_jobs, offset_re, offset_im, gain, audio, n_audio[, stream]); the fake object
# has decimation 4 where nothing else is said, the audio 1024 elements
_A1 = AJ((0, 64, 0))
_MANY = [(0, 1 << 24, i << 24) for i in range(129)]


def _audio(obj=FA(4), pairs=P, n_buffer=512, jobs=_A1, n_jobs=None, off=(0.5, 0.5), gain=1.0, audio=S, n_audio=1024):
    return (obj, pairs, n_buffer, jobs, (len(jobs[1]) if jobs is not None else 0) if n_jobs is None else n_jobs, off[0], off[1], gain, audio,
            n_audio)


_AUDIO_RUN = [
    ("NULL object before the job count", _audio(obj=None, n_jobs=MAX + 1, jobs=None, pairs=None, gain=NAN)),
    ("n_jobs above the maximum", _audio(n_jobs=MAX + 1, jobs=None, pairs=None, gain=NAN)),
    ("no jobs", (FA(4), None, 0, None, 0, NAN, 0.0, NAN, None, 0)),
    ("no jobs, whatever else", (FA(4), P4, 7, None, 0, 0.0, 0.0, 1.0, S1, 0)),
    ("NULL job table", _audio(jobs=None, n_jobs=1, pairs=None, gain=NAN)),
    ("NULL input before the gain", _audio(pairs=None, gain=NAN)),
    ("NULL output before the gain", _audio(audio=None, gain=NAN)),
    ("offset nan before the gain and a span", _audio(off=(NAN, 0.0), gain=NAN, jobs=AJ((600, 1, 0)))),
    ("offset inf before a span", _audio(off=(0.0, INF), jobs=AJ((600, 1, 0)))),
    ("offset -inf before a span", _audio(off=(-INF, 0.0), jobs=AJ((600, 1, 0)))),
    ("gain nan before a span", _audio(gain=NAN, jobs=AJ((600, 1, 0)))),
    ("gain inf before a span", _audio(gain=INF, jobs=AJ((600, 1, 0)))),
    ("gain -inf before a span", _audio(gain=-INF, jobs=AJ((600, 1, 0)))),
    ("job 1 past the buffer", _audio(jobs=AJ((0, 64, 0), (500, 13, 16)))),
    ("first past the buffer", _audio(jobs=AJ((BIG, 1, 0)))),
    ("first + n wraps", _audio(jobs=AJ((2, (1 << 64) - 1, 0)))),
    ("n_pairs too large", _audio(jobs=AJ((0, (1 << 24) + 1, 0)), n_buffer=BIG)),
    ("outputs one past the audio", _audio(jobs=AJ((0, 64, 1009)))),
    ("out_first past the audio", _audio(jobs=AJ((0, 64, BIG)))),
    ("out_first + outputs wraps", _audio(jobs=AJ((0, 64, (1 << 64) - 3)))),
    ("more outputs than the audio", _audio(n_audio=15)),
    ("a span before placement, one job", _audio(jobs=AJ((500, 64, 5000)))),
    ("a span before placement, table order", _audio(jobs=AJ((0, 64, 2000), (BIG, 1, 0)), n_audio=2016)),
    ("placement before a later span", _audio(jobs=AJ((0, 64, 2000), (BIG, 1, 0)))),
    ("jobs 0 and 2 overlap", _audio(jobs=AJ((0, 64, 100), (0, 3, 100), (64, 64, 115), (0, 0, 101)))),
    ("jobs 1 and 2 overlap", _audio(jobs=AJ((0, 64, 100), (8, 64, 50), (64, 64, 50)))),
    ("the audio before overlap", _audio(jobs=AJ((0, 64, 1200), (0, 64, 0), (64, 64, 15)))),
    ("overlap before alignment", _audio(jobs=AJ((0, 64, 116), (64, 64, 101)), pairs=P4)),
    ("the total before alignment", _audio(obj=FA(1), jobs=AJ(*_MANY), n_buffer=BIG, n_audio=BIG, pairs=P4)),
    ("overlap before the total", _audio(obj=FA(1), jobs=AJ(*(_MANY + [(0, 8, 5)])), n_buffer=BIG, n_audio=BIG)),
]
# jobs without output take no room, anywhere, also on top of another
_AEMPTY = AJ((0, 64, 0), (0, 3, 5), (0, 0, 1 << 50))
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
    + _both("fsea_audio_run", _AUDIO_RUN)
    + [("fsea_audio_run_device: alignment behind the jobs' checks", "fsea_audio_run_device", _audio(jobs=_AEMPTY, pairs=P4) + (None,)),
       ("fsea_audio_run_device: input off 8 bytes", "fsea_audio_run_device", _audio(pairs=P4) + (None,)),
       ("fsea_audio_run_device: output off 4 bytes by 2", "fsea_audio_run_device", _audio(audio=S2) + (None,)),
       ("fsea_audio_run_device: input off 1 byte", "fsea_audio_run_device", _audio(pairs=P1) + (None,)),
       ("fsea_audio_run_device: output off 1 byte", "fsea_audio_run_device", _audio(audio=S1) + (None,)),
       ("fsea_audio_layout: fine", "fsea_audio_layout", (FA(4), _AEMPTY, 3, N)),
       ("fsea_audio_layout: NULL object", "fsea_audio_layout", (None, _A1, 1, N)),
       ("fsea_audio_layout: NULL total_outputs", "fsea_audio_layout", (FA(4), _A1, 1, None)),
       ("fsea_audio_layout: NULL job table", "fsea_audio_layout", (FA(4), None, 1, N)),
       ("fsea_audio_layout: n_jobs above the maximum", "fsea_audio_layout", (FA(4), _A1, MAX + 1, N)),
       ("fsea_audio_layout: total_outputs before n_jobs", "fsea_audio_layout", (FA(4), None, MAX + 1, None)),
       ("fsea_audio_layout: object before total_outputs", "fsea_audio_layout", (None, None, MAX + 1, None)),
       ("fsea_audio_layout: no jobs", "fsea_audio_layout", (FA(4), None, 0, N)),
       # fsea_audio_create(out, kind, taps, n_taps, decimation, device): every refusal with everything behind it wrong as well
       ("fsea_audio_create: NULL out-pointer", "fsea_audio_create", (None, 2, None, 0, 0, 99)),
       ("fsea_audio_create: kind 2", "fsea_audio_create", (H, 2, None, 0, 0, 99)),
       ("fsea_audio_create: kind -1", "fsea_audio_create", (H, -1, None, 0, 0, 99)),
       ("fsea_audio_create: NULL taps", "fsea_audio_create", (H, 0, None, 0, 0, 99)),
       ("fsea_audio_create: n_taps 0", "fsea_audio_create", (H, 1, TB, 0, 0, 99)),
       ("fsea_audio_create: n_taps -1", "fsea_audio_create", (H, 1, TB, -1, 0, 99)),
       ("fsea_audio_create: n_taps 513", "fsea_audio_create", (H, 1, TB, 513, 0, 99)),
       ("fsea_audio_create: tap 3 nan", "fsea_audio_create", (H, 1, TB, 21, 0, 99)),
       ("fsea_audio_create: decimation 0", "fsea_audio_create", (H, 1, T, 21, 0, 99)),
       ("fsea_audio_create: decimation -1", "fsea_audio_create", (H, 1, T, 21, -1, 99)),
       ("fsea_audio_create: decimation 65", "fsea_audio_create", (H, 1, T, 21, 65, 99))]
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
    handle, taps, bad = ctypes.c_void_p(), np.ones(21), np.ones(21)
    bad[3] = np.nan
    values = {P: p, P4: p + 4, P1: p + 1, S: p + 4096, S8: p + 4096 + 8, S2: p + 4096 + 2, S1: p + 4096 + 1, N: ctypes.byref(n),
              EV: events.ctypes.data, FT: fits.ctypes.data, FM: ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p),
              H: ctypes.byref(handle), T: taps.ctypes.data, TB: bad.ctypes.data}
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
        if a[0] == "A":
            fake = ctypes.create_string_buffer(4096)
            struct.pack_into("<iiii", fake, 0, 0, 41, a[1], 0)
            alive.append(fake)
            return ctypes.cast(fake, ctypes.c_void_p)
        kind = {"E": fsea.ExtractJob, "M": fsea.MeasureJob, "AJ": fsea.AudioJob}[a[0]]
        alive.append((kind * len(a[1]))(*[kind(*j) for j in a[1]]))
        return ctypes.addressof(alive[-1])

    code = getattr(L, name)(*[value(a) for a in args])
    assert np.all(buf == 0x5A) and not handle.value      # a refused call writes nothing, nor does one without jobs
    return [code, L.fsea_last_error_string().decode() if code else None]


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_is_the_cases(table):
    assert sorted(table) == sorted(IDS)
    # the three objects, device and host form, see each of the shared checks' texts with their own nouns
    shared = ("is NULL", "n_jobs 65537 above 65536", "NULL job table", "NULL buffer", "lie past the", "too large", "more than 2^31")
    for name, nouns in (("fsea_extract_run", ("samples", "of the input", "outputs in one call")),
                        ("fsea_measure_run", ("pairs", "of the buffer", "pairs in one call")),
                        ("fsea_audio_run", ("pairs", "of the buffer", "outputs in one call", "of the audio", "overlap"))):
        for form in ("_device", "_host"):
            texts = " | ".join(t for k, (_, t) in table.items() if k.startswith(name + form + ":") and t)
            for part in shared + nouns:
                assert part in texts, (name + form, part)
            assert [table["%s%s: %s" % (name, form, k)] for k in ("no jobs", "no jobs, whatever else")] == [[0, None], [0, None]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_code_and_text(case, table):
    assert call(case) == table[case[0]]
