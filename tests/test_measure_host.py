"""CPU tier: signal measures without a GPU -- the restatement tests/measure_ref.py against exact arithmetic, inside the bound
the depth of its addition tree gives, and on hand-made special values (a NaN, an infinity, -0.0, the smallest subnormal and
FLT_MAX) against expectations written out by hand; fsea_measure_finish on a tone, on noise and on the NaN cases; fsea_measure_jobs against
its formula; the argument checks of fsea_measure_run_* in the header's order, against a fake object (they read nothing of
it); the shipped kernels' resource usage; fsea-cutouts' new usage error."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import measure_ref as M
from tests.conftest import ROOT
from tests.test_shipped_artifacts import LIB, _kernels

FSEA_EINVAL = -1
TOOL = os.path.join(ROOT, "frequensea_amd", "bin", "fsea-cutouts")
RESULT_FIELDS = ("mean_power", "power_db", "dc_re", "dc_im", "freq_cycles", "coherence", "width_cycles", "kurtosis", "crest")


def as_sums(record):
    """a measure_ref.SUMS scalar as the ctypes record of the binding"""
    return fsea.MeasureSums.from_buffer_copy(np.asarray(record).tobytes())


def noise(seed, n, offset=0j, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.normal(0.0, scale, n) + 1j * rng.normal(0.0, scale, n)) + offset).astype(np.complex64)


def test_header_constants_and_records_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()
    assert int(re.search(r"#define FSEA_MEASURE_TILE_PAIRS (\d+)", text).group(1)) == fsea.MEASURE_TILE_PAIRS == M.TILE == 4096
    assert int(re.search(r"#define FSEA_MEASURE_MAX_JOBS\s+(\d+)", text).group(1)) == fsea.MEASURE_MAX_JOBS == fsea.EXTRACT_MAX_JOBS
    assert re.search(r"#define FSEA_MEASURE_MAX_PAIRS\s+\(1u << 24\)", text) and fsea.MEASURE_MAX_PAIRS == 1 << 24
    assert int(re.search(r"#define FSEA_MEASURE_MAX_LAG\s+(\d+)", text).group(1)) == fsea.MEASURE_MAX_LAG == 65536
    ctype = {"uint64_t": "<u8", "double": "<f8"}
    for c_name, binding, dtype, size in (("fsea_measure_job", fsea.MeasureJob, M.JOB, 16), ("fsea_measure_sums", fsea.MeasureSums, M.SUMS, 80),
                                         ("fsea_measure_result", fsea.MeasureResult, None, 88)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % c_name, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for kind, names in re.findall(r"(uint64_t|double)\s+([\w\s,]+);", body):
            fields += [(n.strip(), ctype[kind]) for n in names.split(",")]
        assert [n for n, _ in fields] == [n for n, _ in binding._fields_], c_name
        assert np.dtype(fields).itemsize == ctypes.sizeof(binding) == size, c_name
        if dtype is not None:
            assert np.dtype(fields) == dtype, c_name
    assert sorted(n for n in fsea.EXPORTS if n.startswith("fsea_measure_")) == [
        "fsea_measure_create", "fsea_measure_destroy", "fsea_measure_finish", "fsea_measure_jobs", "fsea_measure_run_device",
        "fsea_measure_run_host"]


@pytest.mark.parametrize("n,lag", [(1, 1), (300, 1), (4096, 7), (3 * 4096 + 17, 1), (65 * 4096 + 5, 4096)])
def test_the_restatement_lies_within_the_bound_of_its_addition_tree(n, lag):
    """Each of the six sums of measure_ref.sums against the exact sum of the same term values (math.fsum: the exact sum,
    rounded once).

    The bound.  A fold is a fixed tree of additions with acc[0] at its root, and a term passes at most m additions on its way
    there: 16 in its lane of fold_256 (one per step of a tile of 4096), 8 xor stages, then ceil(tiles / 64) in its lane of
    fold_64 and 6 stages more.  Every addition rounds once, relative error at most u = 2^-53, so the computed value is
    sum x_i (1 + e_i) with |e_i| <= (1 + u)^m - 1, and |computed - exact| <= ((1 + u)^m - 1) sum |x_i| < (m + 1) u sum |x_i|
    for these m.  fsum's own rounding is u |exact| <= u sum |x_i|.  (m + 8) u sum |x_i| holds both with room for nothing
    else."""
    offset = 0.5 + 0.5j
    z = noise(n + lag, n, offset)
    t = M.terms(z, offset, lag)
    got = M.sums(z, offset, lag)
    tiles = -(-n // M.TILE)
    m = 16 + 8 + -(-tiles // 64) + 6
    for name, x in zip(M.NAMES, t):
        exact = math.fsum(x.tolist())
        bound = (m + 8) * 2.0 ** -53 * math.fsum(np.abs(x).tolist())
        err = abs(float(got[name]) - exact)
        print(n, lag, name, "error %.3e bound %.3e" % (err, bound))
        assert err <= bound, (n, lag, name, err, bound)
    assert got["peak"] == t[2].max() and got["peak_index"] == int(np.argmax(t[2]))
    assert (got["n_pairs"], got["n_lagged"]) == (n, max(n - lag, 0))
    if lag >= n:
        assert got["r_re"] == 0.0 and got["r_im"] == 0.0
    else:
        assert not np.any(t[4][:lag]) and not np.any(t[5][:lag]) and np.any(t[4][lag:])
    # the order is the contract: the plain left-to-right sum of the same terms is another number
    if n > 4096:
        assert float(got["p"]) != float(np.cumsum(t[2])[-1])


def test_fold_is_the_tree_the_header_describes():
    """fold_W written out for W = 4 on numbers whose sum depends on the order."""
    x = np.array([1.0, 2.0 ** -53, -1.0, 2.0 ** -53, 2.0 ** -52, 1.0, 3.0, -2.0 ** -52, 5.0])
    acc = [0.0 + x[0] + x[4] + x[8], 0.0 + x[1] + x[5], 0.0 + x[2] + x[6], 0.0 + x[3] + x[7]]
    want = (acc[0] + acc[1]) + (acc[2] + acc[3])
    assert M.fold(x, 4) == want
    assert M.fold(np.zeros(0), 256) == 0.0 and M.job_sum(np.zeros(0)) == 0.0
    assert M.fold(np.array([[1.0, 2.0], [3.0, 4.5]]), 64).tolist() == [3.0, 7.5]
    ties = np.zeros(9000, np.complex64)
    assert (M.sums(ties)["peak"], M.sums(ties)["peak_index"]) == (0.0, 0)
    ties[[5000, 77, 8999]] = 2.0
    assert (M.sums(ties)["peak"], M.sums(ties)["peak_index"]) == (4.0, 77)
    empty = M.sums(np.zeros(0, np.complex64), 0.5 + 0.5j, 3)
    assert empty.tobytes() == bytes(80)


# ---- special values: what include/fsea.h promises of a NaN, of -0.0 and of the ends of the f32 range ------------------

TINY, FMAX = 2.0 ** -149, float(np.finfo(np.float32).max)       # the smallest f32 subnormal, FLT_MAX: both exact as doubles
NAMES_AND_PEAK = M.NAMES + ("peak",)


def pairs_f32(re, im):
    """complex64 from two lists through float32 arrays: no complex128 arithmetic between the values and the buffer"""
    z = np.empty(len(re), np.complex64)
    z.real, z.imag = np.asarray(re, np.float32), np.asarray(im, np.float32)
    return z


def special_sums(z, offset=0j, lag=1):
    """measure_ref.sums where inf - inf and inf * 0 are meant"""
    with np.errstate(invalid="ignore", over="ignore"):
        return M.sums(z, offset, lag)


def bits_of(x):
    return int(np.float64(x).view(np.uint64))


def extremes_buffer(n, at):
    """n pairs: in front of `at` small whole multiples of the smallest f32 subnormal (every sum of them is exact in f64 and
    is 0 if a conversion flushes), from `at` on +-FLT_MAX (|z|^4 = 2^514 a pair: finite in f64 over any job)."""
    k = np.arange(n)
    re, im = ((k % 3) + 1) * TINY * (1 - 2 * (k % 2)), ((k % 5) - 2) * TINY
    re[at:], im[at:] = FMAX * (1 - 2 * (k[at:] % 2)), FMAX * (1 - 2 * ((k[at:] // 2) % 2))
    return pairs_f32(re, im)


@pytest.mark.parametrize("n", [1, 257, 2 * M.TILE + 1])
def test_minus_zero_pairs_give_plus_zero_sums(n):
    """a = -0.0 - +0.0 = -0.0 in every term of s_re and s_im; an accumulator that starts at +0.0 stays +0.0 under it, "so an
    absent term may be added as +0.0 or left out"."""
    z = pairs_f32([-0.0] * n, [-0.0] * n)
    assert np.all(np.signbit(z.real)) and np.all(np.signbit(z.imag))
    a, b = M.terms(z, 0j, 1)[:2]
    assert np.all(np.signbit(a)) and np.all(np.signbit(b))                         # the terms are -0.0 ...
    for lag in (1, 7):
        s = special_sums(z, 0j, lag)
        for name in NAMES_AND_PEAK:
            assert bits_of(s[name]) == 0, (n, lag, name)                           # ... and every sum +0.0 by its bits
        assert (s["peak_index"], s["n_pairs"], s["n_lagged"]) == (0, n, max(n - lag, 0))


def test_a_nan_term_poisons_its_sums_and_is_never_the_peak():
    z = pairs_f32([1.0, np.nan, 3.0, 0.5], [1.0, 2.0, -2.0, 0.0])
    clean = pairs_f32([1.0, 0.0, 3.0, 0.5], [1.0, 2.0, -2.0, 0.0])
    s, c = special_sums(z), special_sums(clean)
    assert s["s_im"] == 1.0 and bits_of(s["s_im"]) == bits_of(c["s_im"])           # 1 + 2 - 2 + 0
    for name in ("s_re", "p", "q", "r_re", "r_im"):
        assert np.isnan(s[name]) and np.isfinite(c[name]), name
    assert (s["peak"], s["peak_index"]) == (13.0, 2) == (c["peak"], c["peak_index"])      # 3^2 + 2^2, the other pairs' largest
    # the NaN in front of the largest, behind it, first and last: the same peak; in its place: the next largest
    for k in range(4):
        z = pairs_f32([1.0, 2.0, 3.0, 0.5], [1.0, 2.0, -2.0, 0.0])
        z.real[k] = np.nan
        want = (13.0, 2) if k != 2 else (8.0, 1)
        assert (special_sums(z)["peak"], special_sums(z)["peak_index"]) == want, k
    # lag 2: the partner's NaN reaches r two pairs on, nothing else changes
    s = special_sums(pairs_f32([1.0, np.nan, 3.0, 0.5], [1.0, 2.0, -2.0, 0.0]), 0j, 2)
    assert np.isnan(s["r_re"]) and np.isnan(s["r_im"]) and s["s_im"] == 1.0 and s["n_lagged"] == 2
    # all NaN: peak +0.0 at index 0, as an empty or a silent job
    s = special_sums(pairs_f32([np.nan] * 5, [np.nan] * 5))
    assert bits_of(s["peak"]) == 0 and s["peak_index"] == 0 and all(np.isnan(s[name]) for name in M.NAMES)


def test_an_infinity_is_the_peak_at_its_index():
    s = special_sums(pairs_f32([1.0, 2.0, 3.0], [1.0, np.inf, 0.5]))
    assert s["p"] == np.inf and s["q"] == np.inf and (s["peak"], s["peak_index"]) == (np.inf, 1)
    assert s["s_re"] == 6.0 and s["s_im"] == np.inf
    assert s["r_re"] == np.inf and np.isnan(s["r_im"])        # r_re: 2 * 1 + inf * 1, 3 * 2 + 0.5 * inf; r_im of pair 1 and 2: inf, -inf


def test_the_ends_of_the_f32_range_give_finite_sums_computed_by_hand():
    """The smallest subnormal and FLT_MAX are exact doubles and so are their products here; the folds of two and three terms
    are (x0 + x1) and (x0 + x1) + (x2 + 0), everything else of the tree adds +0.0."""
    t, F = TINY, FMAX
    s = special_sums(pairs_f32([t, 3 * t], [-t, t]))
    want = {"s_re": t + 3 * t, "s_im": -t + t, "p": (t * t + t * t) + (9 * t * t + t * t), "q": (2 * t * t) ** 2 + (10 * t * t) ** 2,
            "r_re": 0.0 + (3 * t * t + t * -t), "r_im": 0.0 + (t * t - 3 * t * -t), "peak": 10 * t * t}
    for name in NAMES_AND_PEAK:
        assert bits_of(s[name]) == bits_of(want[name]) and np.isfinite(s[name]), (name, s[name], want[name])
    assert s["p"] == 12 * 2.0 ** -298 > 0.0 and s["s_re"] == 2.0 ** -147 and s["peak_index"] == 1
    s = special_sums(pairs_f32([F, -F, t], [F, F, F]))
    want = {"s_re": (F + -F) + (t + 0.0), "s_im": (F + F) + (F + 0.0), "p": (2 * F * F + 2 * F * F) + ((t * t + F * F) + 0.0),
            "q": ((2 * F * F) ** 2 + (2 * F * F) ** 2) + ((t * t + F * F) ** 2 + 0.0),
            "r_re": (0.0 + (-F * F + F * F)) + ((t * -F + F * F) + 0.0), "r_im": (0.0 + (F * F - -F * F)) + ((F * -F - t * F) + 0.0),
            "peak": 2 * F * F}
    for name in NAMES_AND_PEAK:
        assert bits_of(s[name]) == bits_of(want[name]) and np.isfinite(s[name]), (name, s[name], want[name])
    assert s["s_re"] == t and s["peak_index"] == 0 and s["q"] > 2.0 ** 515
    # the buffer of the GPU tier: subnormals alone in front (exact sums, none of them zero), FLT_MAX behind, all finite
    z = extremes_buffer(700, 400)
    assert np.all(np.abs(z[:400].real) >= TINY) and np.all(np.abs(z[:400].real) <= 3 * TINY) and np.all(np.abs(z[400:].real) == FMAX)
    s = special_sums(z[:257], 0j, 7)
    k = np.arange(257)
    assert s["s_re"] == float(np.sum(((k % 3) + 1) * (1 - 2 * (k % 2)))) * t != 0.0 and s["p"] > 0.0 and s["q"] > 0.0 and s["r_re"] != 0.0
    for a, n in ((0, 700), (300, 257), (400, 300), (399, 2)):
        s = special_sums(z[a:a + n], 0j, 1)
        assert all(np.isfinite(s[name]) for name in NAMES_AND_PEAK), (a, n, s)


@pytest.mark.parametrize("lag", [1, 3])
def test_finish_on_a_pure_tone(lag):
    """e^(2 pi j f i) rounded to f32, f = 0.0371: the frequency within 1e-6 (ten times the worst phase error of one f32 sample,
    2^-24 / (2 pi) ~ 1e-8 cycles, which the sum over 20000 pairs only averages down), a constant envelope and one line."""
    f, n = 0.0371, 20000
    z = np.exp(2j * np.pi * f * np.arange(n)).astype(np.complex64)
    r = fsea.measure_finish(as_sums(M.sums(z, 0j, lag)), lag)
    print(lag, r.freq_cycles, r.kurtosis, r.coherence, r.width_cycles)
    assert abs(r.freq_cycles - f) <= 1e-6
    assert abs(r.kurtosis - 1.0) <= 1e-6 and abs(r.coherence - 1.0) <= 1e-6 and 0.0 <= r.width_cycles < 1e-3
    assert abs(r.mean_power - 1.0) <= 1e-6 and abs(r.power_db) <= 1e-5 and abs(r.crest - 1.0) <= 1e-6
    assert r.n_pairs == n and r.peak_index < n


@pytest.mark.parametrize("lag", [1, 5])
def test_finish_on_noise_is_its_formulas(lag):
    """Every field against the same formulas in numpy, to 1e-12 relative; the statistics themselves only loosely."""
    z = noise(7, 30000, 0.25 - 0.125j, 3.0)
    s = M.sums(z, 0j, lag)
    r = fsea.measure_finish(as_sums(s), lag)
    want = M.finish(s, lag)
    for name in RESULT_FIELDS:
        got = getattr(r, name)
        assert abs(got - want[name]) <= 1e-12 * abs(want[name]), (name, got, want[name])
    assert (r.peak_index, r.n_pairs) == (want["peak_index"], want["n_pairs"]) == (int(s["peak_index"]), 30000)
    assert 1.9 < r.kurtosis < 2.1 and r.coherence < 0.1 and r.crest > 4.0
    assert abs(r.dc_re - 0.25) < 0.1 and abs(r.dc_im + 0.125) < 0.1


def test_finish_gives_nan_where_there_is_nothing_to_divide_by():
    L = fsea.hip_lib()
    empty = fsea.measure_finish(as_sums(M.sums(np.zeros(0, np.complex64))), 1)
    for name in RESULT_FIELDS:
        assert math.isnan(getattr(empty, name)), name
    assert (empty.peak_index, empty.n_pairs) == (0, 0)
    silent = fsea.measure_finish(as_sums(M.sums(np.zeros(100, np.complex64))), 1)
    assert silent.mean_power == 0.0 and silent.power_db == -math.inf and silent.dc_re == 0.0 and silent.dc_im == 0.0
    for name in ("kurtosis", "crest", "coherence", "width_cycles"):
        assert math.isnan(getattr(silent, name)), name
    short = fsea.measure_finish(as_sums(M.sums(noise(3, 4), 0j, 4)), 4)          # n == lag: nothing lagged
    assert short.n_pairs == 4 and short.mean_power > 0.0 and short.kurtosis >= 1.0
    for name in ("freq_cycles", "coherence", "width_cycles"):
        assert math.isnan(getattr(short, name)), name
    s, r = fsea.MeasureSums(), fsea.MeasureResult()
    assert L.fsea_measure_finish(None, 1, ctypes.byref(r)) == FSEA_EINVAL and b"NULL" in L.fsea_last_error_string()
    assert L.fsea_measure_finish(ctypes.byref(s), 1, None) == FSEA_EINVAL
    for lag in (0, -1, fsea.MEASURE_MAX_LAG + 1):
        assert L.fsea_measure_finish(ctypes.byref(s), lag, ctypes.byref(r)) == FSEA_EINVAL and b"lag" in L.fsea_last_error_string()
    assert L.fsea_measure_finish(ctypes.byref(s), fsea.MEASURE_MAX_LAG, ctypes.byref(r)) == 0


def test_measure_jobs_is_its_formula():
    L = fsea.hip_lib()
    ns = [0, 15, 16, 17, 16 * 6, 16 * 7 - 1, 16 * 7, 16 * 1000 + 3, 5]
    ejobs = [fsea.ExtractJob(3 * i, n, 0, 0.0, 0.0, 1000 * i + 2) for i, n in enumerate(ns)]
    for d, skip in ((16, 6), (16, 0), (1, 6), (5, 1 << 40)):
        got = np.frombuffer(fsea.measure_jobs(ejobs, d, skip), dtype=M.JOB)
        want = M.measure_jobs(ejobs, d, skip)
        assert np.array_equal(got, want), (d, skip)
    d16 = np.frombuffer(fsea.measure_jobs(ejobs, 16, 6), dtype=M.JOB)
    assert d16[0].tolist() == (2, 0) and d16[4].tolist() == (4002 + 6, 0) and d16[5].tolist() == (5002 + 6, 0)     # skip >= outputs
    assert d16[6].tolist() == (6002 + 6, 1) and d16[7].tolist() == (7002 + 6, 994)
    assert len(fsea.measure_jobs([], 16, 6)) == 0
    one = (fsea.ExtractJob * 2)(fsea.ExtractJob(0, 64, 0, 0.0, 0.0, 0), fsea.ExtractJob(0, (1 << 24) + 8, 0, 0.0, 0.0, 0))
    out = (fsea.MeasureJob * 2)()
    a, o = ctypes.addressof(one), ctypes.addressof(out)
    assert L.fsea_measure_jobs(a, 2, 1, 7, o) == FSEA_EINVAL and b"job 1" in L.fsea_last_error_string()
    assert L.fsea_measure_jobs(a, 2, 1, 8, o) == 0 and out[1].n_pairs == 1 << 24
    assert L.fsea_measure_jobs(a, 2, 0, 0, o) == FSEA_EINVAL and b"decimation" in L.fsea_last_error_string()
    assert L.fsea_measure_jobs(None, 2, 1, 0, o) == FSEA_EINVAL and L.fsea_measure_jobs(a, 2, 1, 0, None) == FSEA_EINVAL
    assert L.fsea_measure_jobs(a, fsea.MEASURE_MAX_JOBS + 1, 1, 0, o) == FSEA_EINVAL and b"n_jobs" in L.fsea_last_error_string()
    assert L.fsea_measure_jobs(None, 0, 1, 0, None) == 0


def test_measure_rejects_bad_arguments_without_a_device_in_the_headers_order():
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    h = ctypes.c_void_p()
    assert L.fsea_measure_create(None, 0) == FSEA_EINVAL and b"out-pointer" in err()
    assert L.fsea_measure_destroy(None) == 0
    buf = np.full(8192, 0x5A, np.uint8)
    p = buf.ctypes.data
    assert p % 16 == 0
    sums = p + 4096
    fake = ctypes.create_string_buffer(4096)          # the checks read nothing of the object
    f = ctypes.cast(fake, ctypes.c_void_p)
    big = 1 << 40

    def table(*jobs):
        return (fsea.MeasureJob * len(jobs))(*[fsea.MeasureJob(a, n) for a, n in jobs])

    one = table((0, 64))
    forms = ((L.fsea_measure_run_device, (None,)), (L.fsea_measure_run_host, ()))

    def refused(word, obj=f, pairs=p, n_buffer=512, jobs=one, off=(0.5, 0.5), lag=1, out=sums, only=None, n_jobs=None):
        for run, tail in forms:
            if only is not None and run is not only:
                continue
            rc = run(obj, pairs, n_buffer, ctypes.addressof(jobs) if jobs is not None else None, len(jobs) if n_jobs is None else n_jobs,
                     off[0], off[1], lag, out, *tail)
            assert rc == FSEA_EINVAL and word in err(), (run, word, err())

    # every refusal with everything behind it in the order wrong as well: the earlier check speaks
    refused(b"measure is NULL", obj=None, n_jobs=fsea.MEASURE_MAX_JOBS + 1, jobs=None, pairs=None, lag=0)
    refused(b"n_jobs", n_jobs=fsea.MEASURE_MAX_JOBS + 1, jobs=None, pairs=None, lag=0)
    for run, tail in forms:                                # no jobs: a no-op whatever else is given
        assert run(f, None, 0, None, 0, np.nan, 0.0, 0, None, *tail) == 0
        assert run(f, p + 4, 7, None, 0, 0.0, 0.0, 1, sums + 8, *tail) == 0
    refused(b"NULL job table", jobs=None, n_jobs=1, pairs=None, lag=0)
    refused(b"NULL buffer", pairs=None, lag=0)
    refused(b"NULL buffer", out=None, lag=0)
    for lag in (0, -3, fsea.MEASURE_MAX_LAG + 1):
        refused(b"lag", lag=lag, off=(np.nan, 0.0))
    for off in ((np.nan, 0.0), (0.0, np.inf), (-np.inf, 0.0)):
        refused(b"offset", off=off, jobs=table((600, 1)))
    two = table((0, 64), (500, 13))
    refused(b"job 1: pairs", jobs=two)                                   # past the buffer
    refused(b"job 0: pairs", jobs=table((big, 1)))
    refused(b"job 0: pairs", jobs=table((2, (1 << 64) - 1)))                       # first + n wraps
    refused(b"job 0: n_pairs", jobs=table((0, (1 << 24) + 1)), n_buffer=big)
    refused(b"job 1: pairs", jobs=table((0, 1 << 24), (big, 1)), n_jobs=2, n_buffer=big)
    many = table(*[(0, 1 << 24)] * 129)
    refused(b"more than 2^31", jobs=many, n_buffer=big, pairs=p + 4)   # the total before alignment
    late = table(*([(0, 1 << 24)] * 129 + [(big, 1)]))
    refused(b"job 129: pairs", jobs=late, n_buffer=big)                # a job before the total
    for d_pairs, d_sums in ((p + 4, sums), (p, sums + 8), (p + 1, sums)):
        refused(b"aligned", pairs=d_pairs, out=d_sums, only=L.fsea_measure_run_device)
    assert np.all(buf == 0x5A)                                                                      # a refused call writes nothing
    rc = L.fsea_measure_create(ctypes.byref(h), 0)
    if fsea.device_count() == 0:
        assert rc == -2 and not h.value                                                             # FSEA_ENODEVICE
    else:
        assert rc == 0 and L.fsea_measure_destroy(h) == 0


def test_shipped_library_has_the_measure_kernels_within_their_budget():
    """fsea_measure_tiles and fsea_measure_fold from the code object's metadata alone: wave64, no scratch, no spilled register;
    the tile kernel within 128 VGPRs, so four of its workgroups' waves share a SIMD, and no more registers than the build it
    was written against; the fold a single wave without LDS."""
    assert os.path.exists(LIB), "libfsea_hip.so not built"
    ks = _kernels(LIB)
    for name, wg, vgprs, sgprs, lds in (("fsea_measure_tiles", 256, TILES_VGPRS, TILES_SGPRS, 256), ("fsea_measure_fold", 64, FOLD_VGPRS, FOLD_SGPRS, 0)):
        k = ks[name]
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"],
              k[".vgpr_spill_count"], k[".sgpr_spill_count"])
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == wg, name
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= vgprs and k[".sgpr_count"] <= sgprs, (name, k[".vgpr_count"], k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == lds, name


TILES_VGPRS, TILES_SGPRS, FOLD_VGPRS, FOLD_SGPRS = 128, 64, 48, 32      # read off the build: 104 and 50, 39 and 28


def test_tool_refuses_a_lag_outside_its_range():
    assert os.path.exists(TOOL), "fsea-cutouts not built"
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--measures [--lag K]" in r.stdout
    x = ["x.raw", "--size", "1024", "--out", "y", "--decimation", "4", "--measures"]
    for lag in ("0", "65537", "-1"):
        r = subprocess.run([TOOL] + x + ["--lag", lag], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--lag must be in [1, 65536]" in r.stderr and r.stderr.startswith("fsea-cutouts: "), r.stderr
