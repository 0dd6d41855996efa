"""GPU tier: signal measures (fsea_measure_*, kernels fsea_measure_tiles and fsea_measure_fold) and fsea-cutouts --measures.

Bit identity, no tolerance: a job's record is tests/measure_ref.py's for the job's pairs -- the same terms with the same
roundings, fold_256 inside a tile and fold_64 over the tiles -- whatever first_pair is, whatever other jobs share the call
and in whatever order.  The shapes are the smallest at which the kernels can still go wrong: lengths round the lag, a wave,
a workgroup's 256 lanes, one and two tiles, the 64 tiles of the fold's first round; odd and even firsts; jobs that overlap;
one that ends with the buffer; a table long enough for the bisection to take every turn.  Inputs and outputs are guarded.

Special values, where the header promises something (a NaN term is never the peak, an accumulator is never -0.0, the terms are
f64 conversions of the f32 values): one NaN or infinity per buffer at every place a kernel treats differently -- the stand-ins
of a missing partner and of pairs past the end, both bodies, the lane's chain, the combine's and the fold's peak merges --,
a buffer of -0.0, and one of subnormals and FLT_MAX.  Records that hold NaNs are compared through same_record; every other
test keeps same_record_bits."""
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import extract_ref as R
from tests import measure_ref as M
from tests.conftest import ROOT
from tests.guarded import FILL, Guarded
from tests.jobs_common import address, pairs_of, pedestal, same_record_bits
from tests.test_measure_host import extremes_buffer, pairs_f32, special_sums

pytestmark = pytest.mark.gpu

T = fsea.MEASURE_TILE_PAIRS
OFFSET = 0.5 + 0.5j
BIN = os.path.join(ROOT, "frequensea_amd", "bin")
FSEA_EINVAL = -1


def lengths(lag):
    return [0, 1, lag, lag + 1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 63 * T, 64 * T + 1]


def sweep(lag):
    """(jobs as (first, n), n_buffer): every length at an even and at an odd first, all of them overlapping in the buffer's
    first pairs; the longest job at an odd first ends with the buffer."""
    ns = lengths(lag)
    jobs = []
    for i, n in enumerate(ns):
        jobs.append((2 * (len(ns) - i), n))
        jobs.append((2 * i + 1, n))
    n_buffer = max(a + n for a, n in jobs)
    assert sum(1 for a, n in jobs if a + n == n_buffer and a % 2 == 1 and n == 64 * T + 1) == 1
    return jobs, n_buffer


def table(jobs):
    return (fsea.MeasureJob * len(jobs))(*[fsea.MeasureJob(a, n) for a, n in jobs])


def run_device(m, d_pairs, n_buffer, jobs, lag, offset=OFFSET, stream=0, wait=None):
    """one call into a guarded output -> the records as an array of M.SUMS; the guard bands are checked"""
    g = Guarded(80 * len(jobs))
    m.run_device(d_pairs.addr, n_buffer, table(jobs), g.addr, offset=offset, lag=lag, stream=stream)
    if wait is not None:
        wait()
    got = g.payload(M.SUMS, (len(jobs),))
    g.check("the records of %d jobs" % len(jobs))
    g.free()
    return got


@pytest.fixture(scope="module")
def resident():
    """the buffer of the sweeps, on the device once: (host pairs, guarded device copy)"""
    _, n_buffer = sweep(4096)
    z = pairs_of(20, n_buffer)
    d = Guarded(z.nbytes).upload(z)
    yield z, d
    d.check("the input is read, not written")
    d.free()


@pytest.mark.parametrize("lag", [1, 7, 4096])
def test_every_record_equals_the_restatement_bit_for_bit(resident, lag):
    z, d_pairs = resident
    jobs, n_buffer = sweep(lag)
    assert n_buffer == z.size
    m = fsea.Measure()
    got = run_device(m, d_pairs, n_buffer, jobs, lag)
    for k, (a, n) in enumerate(jobs):
        want = M.sums(z[a:a + n], OFFSET, lag)
        assert same_record_bits(got[k], want), (lag, k, a, n, got[k], want)
    assert got["n_pairs"].tolist() == [n for _, n in jobs] and got["n_lagged"].tolist() == [max(n - lag, 0) for _, n in jobs]
    # the host form: the same bytes
    host = np.frombuffer(m.run(z, table(jobs), OFFSET, lag), dtype=M.SUMS)
    assert same_record_bits(host, got), lag
    m.close()


def test_the_table_does_not_change_a_bit(resident):
    """The same jobs permuted, each alone in a call, and scattered among 700 one-tile jobs: identical bytes per job."""
    z, d_pairs = resident
    lag = 7
    jobs, n_buffer = sweep(lag)
    m = fsea.Measure()
    together = run_device(m, d_pairs, n_buffer, jobs, lag)
    order = list(np.random.default_rng(6).permutation(len(jobs)))
    permuted = run_device(m, d_pairs, n_buffer, [jobs[k] for k in order], lag)
    for at, k in enumerate(order):
        assert same_record_bits(permuted[at], together[k]), k
    for k, j in enumerate(jobs):
        alone = run_device(m, d_pairs, n_buffer, [j], lag)
        assert same_record_bits(alone[0], together[k]), k
    # 700 jobs of one tile each (every ninth one empty), the sweep's jobs between them every 27th place
    small = [(11 * i + i % 2, 0 if i % 9 == 4 else 40 + (i * 131) % 4000) for i in range(700)]
    big, where = list(small), {}
    for k, j in enumerate(jobs):
        at = 27 * k + k
        big.insert(at, j)
        where[k] = at
    assert all(big[at] == jobs[k] for k, at in where.items()) and len(big) == 700 + len(jobs)
    among = run_device(m, d_pairs, n_buffer, big, lag)
    for k, at in where.items():
        assert same_record_bits(among[at], together[k]), k
    placed = set(where.values())
    for at, (a, n) in enumerate(big):                       # and the small ones are right too
        if at not in placed:
            assert same_record_bits(among[at], M.sums(z[a:a + n], OFFSET, lag)), (at, a, n)
    m.close()


def test_the_first_of_equal_peaks_wins():
    """Two equal maxima in two tiles, in two lanes, in one lane's two steps, in two waves: peak_index is the first; a job of
    equal pairs gives 0, an empty one zeros, a silent one peak +0.0 at 0."""
    a, n = 3, 2 * T + 77                                    # an odd first: the tiles are the job's own, not the buffer's
    m = fsea.Measure()
    for name, (i0, i1) in {"two tiles": (9000, 5000), "two lanes": (300, 808), "one lane": (40, 296), "two waves": (130, 70)}.items():
        z = np.full(3 * T + 100, 0.25 + 0.25j, np.complex64)
        z[a + i0] = z[a + i1] = 3.0 - 2.0j
        d = Guarded(z.nbytes).upload(z)
        got = run_device(m, d, z.size, [(a, n), (a, 30), (0, 0)], 1, offset=0j)
        ref = M.sums(z[a:a + n], 0j, 1)
        assert got[0]["peak"] == 13.0 and got[0]["peak_index"] == min(i0, i1) == ref["peak_index"], (name, got[0])
        assert same_record_bits(got[0], ref), name
        assert (got[1]["peak"], got[1]["peak_index"]) == (0.125, 0), name           # all equal: the first
        assert got[2].tobytes() == bytes(80), name                                   # empty: zeros, peak +0.0
        d.check(name)
        d.free()
    zeros = np.zeros(T + 5, np.complex64)
    d = Guarded(zeros.nbytes).upload(zeros)
    got = run_device(m, d, zeros.size, [(1, T + 4)], 1, offset=0j)
    assert (got[0]["peak"], got[0]["peak_index"], got[0]["p"]) == (0.0, 0, 0.0)
    d.free()
    m.close()


def test_refusals_name_the_job_and_write_nothing(resident):
    z, d_pairs = resident
    L = fsea.hip_lib()
    err = L.fsea_last_error_string
    m = fsea.Measure()
    g = Guarded(80 * 4)
    n_buffer = z.size

    def refused(word, jobs, pairs=d_pairs.addr, n=n_buffer, off=(0.5, 0.5), lag=1, out=g.addr, obj=None, n_jobs=None):
        tab = table(jobs) if jobs is not None else None
        rc = L.fsea_measure_run_device(m._p if obj is None else obj, pairs, n, address(tab), len(jobs) if n_jobs is None else n_jobs,
                                       off[0], off[1], lag, out, None)
        assert rc == FSEA_EINVAL and word in err(), (word, rc, err())

    ok = [(0, 10), (5, 20)]
    assert L.fsea_measure_run_device(None, d_pairs.addr, n_buffer, address(table(ok)), 2, 0.5, 0.5, 1, g.addr, None) == FSEA_EINVAL
    assert b"measure is NULL" in err()
    refused(b"n_jobs", ok, n_jobs=fsea.MEASURE_MAX_JOBS + 1)
    refused(b"NULL job table", None, n_jobs=2)
    refused(b"NULL buffer", ok, pairs=None)
    refused(b"NULL buffer", ok, out=None)
    refused(b"lag", ok, lag=0)
    refused(b"lag", ok, lag=fsea.MEASURE_MAX_LAG + 1)
    refused(b"offset", ok, off=(np.nan, 0.5))
    refused(b"offset", ok, off=(0.5, np.inf))
    refused(b"job 1: pairs", [(0, 10), (n_buffer - 19, 20)])
    refused(b"job 2: pairs", [(0, 10), (5, 20), (n_buffer + 1, 0)])
    refused(b"job 1: n_pairs", [(0, 10), (0, fsea.MEASURE_MAX_PAIRS + 1)], n=1 << 30)
    refused(b"more than 2^31", [(0, 1 << 24)] * 129, n=1 << 30)
    refused(b"aligned", ok, pairs=d_pairs.addr + 4)
    refused(b"aligned", ok, out=g.addr + 8)
    assert L.fsea_measure_run_device(m._p, None, 0, None, 0, np.nan, 0.0, 0, None, None) == 0          # no jobs: a no-op
    assert np.all(g.payload(np.uint8, (320,)) == FILL)
    g.check("refused calls")
    # and the same object still works, at the edge of what is accepted: a job that ends with the buffer, the largest lag
    got = run_device(m, d_pairs, n_buffer, [(n_buffer - 20, 20), (n_buffer, 0)], fsea.MEASURE_MAX_LAG)
    assert same_record_bits(got[0], M.sums(z[n_buffer - 20:], OFFSET, fsea.MEASURE_MAX_LAG)) and got[1].tobytes() == bytes(80)
    g.free()
    m.close()


def test_two_streams_and_an_odd_pair_base(resident):
    """Two calls with different tables queued back to back on two streams: each its own result (the object's table and
    partials are shared, an event orders the calls).  A buffer that begins at an odd pair of the allocation: 8-byte aligned
    is all d_pairs has to be."""
    z, d_pairs = resident
    m = fsea.Measure()
    sync = fsea.Plan(128)                        # fsea_stream_synchronize wants a plan for its device
    s1, s2 = fsea.Stream(), fsea.Stream()
    jobs_a = [(1, 3 * T + 5), (10, 300)]
    jobs_b = [(2, 70), (7, 2 * T), (0, 0), (4, T + 1)]
    g_a, g_b = Guarded(80 * len(jobs_a)), Guarded(80 * len(jobs_b))
    m.run_device(d_pairs.addr, z.size, table(jobs_a), g_a.addr, offset=OFFSET, lag=3, stream=s1)
    m.run_device(d_pairs.addr + 8, z.size - 1, table(jobs_b), g_b.addr, offset=OFFSET, lag=2, stream=s2)
    sync.synchronize(s1)
    sync.synchronize(s2)
    got_a, got_b = g_a.payload(M.SUMS, (len(jobs_a),)), g_b.payload(M.SUMS, (len(jobs_b),))
    for k, (a, n) in enumerate(jobs_a):
        assert same_record_bits(got_a[k], M.sums(z[a:a + n], OFFSET, 3)), k
    for k, (a, n) in enumerate(jobs_b):
        assert same_record_bits(got_b[k], M.sums(z[1 + a:1 + a + n], OFFSET, 2)), k
    for g in (g_a, g_b):
        g.check("two streams")
        g.free()
    for o in (s1, s2, sync, m):
        o.close()


# ---- special values: a NaN, an infinity, -0.0 and the ends of the f32 range, where the header promises something --------

N_SPECIAL = 3 * T + 300
SPECIAL_LENGTHS = (1, 257, 2 * T, 2 * T + 1)     # the second tile of the longer two takes the body without tests
SPECIAL_FIRSTS = (4, 7)
SPECIAL_LAGS = (1, 7)
LOUD = np.complex64(40.5 - 29.5j)                # |z - OFFSET|^2 = 2500: far above any of the Gaussian pairs


def same_record(got, want):
    """The comparison rule for records that hold NaNs: peak, peak_index, n_pairs and n_lagged by their bits; each of the six
    sums by its bits where the reference is not a NaN and "is a NaN" where it is -- neither include/fsea.h nor IEEE 754 fixes
    the sign and the payload of a generated NaN, and x86 and the GPU differ."""
    ok = all(same_record_bits(got[name], want[name]) for name in ("peak", "peak_index", "n_pairs", "n_lagged"))
    for name in M.NAMES:
        ok = ok and (bool(np.isnan(got[name])) if np.isnan(want[name]) else same_record_bits(got[name], want[name]))
    return ok


def placements(n):
    """{name: (index of the special pair, index of a planted maximum or None)} inside a job of n pairs"""
    out = {"a: pair 0, the stand-in for a missing partner": (0, None)}
    if n == 1:
        return out
    if n % T:
        out["b: the last pair of a ragged tile, the stand-in for pairs past the end"] = (n - 1, None)
    out["c: a middle lane of tile 0"] = (100 if n < 1000 else 868, None)
    if n >= 2 * T:
        out["d: inside the whole second tile"] = (T + 1500, None)
        for base, body in ((0, "tile 0"), (T, "the whole second tile")):
            out["e: 256 pairs in front of the maximum, in its lane's column, %s" % body] = (base + 1068, base + 1324)
            out["e: 256 pairs behind the maximum, in its lane's column, %s" % body] = (base + 1580, base + 1324)
        out["f: in another wave than the maximum"] = (200, 70)
        out["f: in the tile behind the maximum's"] = (T + 10, 70)
        out["f: in the tile in front of the maximum's"] = (70, T + 10)
    else:
        out["e: 256 pairs in front of the maximum, in its lane's column"] = (0, 256)
        out["e: 256 pairs behind the maximum, in its lane's column"] = (256, 0)
        out["f: in another wave than the maximum"] = (200, 70)
    return out


def neighbours(first, n, at):
    """the jobs inside (first, n) that end just in front of pair `at` of it or begin just behind it"""
    return [(a, m) for a, m in ((first, at), (first + at + 1, n - at - 1)) if m > 0]


@pytest.fixture(scope="module")
def special():
    """(the Gaussian buffer the special pairs are planted in, a guarded device buffer of its size, a Measure)"""
    z = pairs_of(21, N_SPECIAL)
    d = Guarded(z.nbytes)
    m = fsea.Measure()
    yield z, d, m
    d.check("the input is read, not written")
    d.free()
    m.close()


@pytest.mark.parametrize("n", SPECIAL_LENGTHS)
@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_a_nan_or_an_infinity_at_every_place_a_kernel_treats_differently(special, kind, n):
    """One special pair per buffer (a NaN in re, +inf in im) at each place of `placements`, in a job at an even and at an odd
    first_pair, with lags 1 and 7: the record is measure_ref.sums' by same_record; the peak is that of the other pairs (the
    NaN) or the special pair's (the infinity); the jobs on either side of the special pair are finite and bit-identical."""
    base, d_pairs, m = special
    for first in SPECIAL_FIRSTS:
        for name, (at, loud) in placements(n).items():
            z = base.copy()
            if loud is not None:
                z[first + loud] = LOUD
            if kind == "nan":
                z.real[first + at] = np.nan
            else:
                z.imag[first + at] = np.inf
            d_pairs.upload(z)
            jobs = [(first, n)] + neighbours(first, n, at)
            for lag in SPECIAL_LAGS:
                what = (kind, n, first, lag, name)
                got = run_device(m, d_pairs, N_SPECIAL, jobs, lag)
                want = [special_sums(z[a:a + k], OFFSET, lag) for a, k in jobs]
                assert same_record(got[0], want[0]), what + (got[0], want[0])
                if kind == "nan":
                    assert np.isnan(got[0]["s_re"]) and np.isnan(got[0]["p"]) and np.isnan(got[0]["q"]), what
                    assert np.isfinite(got[0]["s_im"]) and np.isfinite(got[0]["peak"]), what
                    others = np.delete(z[first:first + n], at).astype(np.complex128) - OFFSET
                    power = others.real * others.real + others.imag * others.imag
                    if n > 1:
                        k = int(np.argmax(power))
                        assert (got[0]["peak"], got[0]["peak_index"]) == (power[k], k + (k >= at)), what
                    else:
                        assert got[0]["peak"].tobytes() == bytes(8) and got[0]["peak_index"] == 0, what     # all NaN: +0.0 at 0
                    if loud is not None:
                        assert (got[0]["peak"], got[0]["peak_index"]) == (2500.0, loud), what
                else:
                    assert (got[0]["p"], got[0]["q"], got[0]["peak"], got[0]["peak_index"]) == (np.inf, np.inf, np.inf, at), what
                for k in range(1, len(jobs)):
                    assert same_record_bits(got[k], want[k]), what + (jobs[k],)
                    assert all(np.isfinite(got[k][f]) for f in M.NAMES + ("peak",)), what + (jobs[k],)
                host = np.frombuffer(m.run(z, table(jobs), OFFSET, lag), dtype=M.SUMS)
                assert all(same_record(host[k], want[k]) for k in range(len(jobs))), what + ("host form",)


def test_minus_zero_pairs_give_plus_zero_records(special):
    """Every pair -0.0 - 0.0j with offset +0.0: the terms of s_re and s_im are -0.0, an absent one is +0.0, and every sum and
    the peak are +0.0 by their bits at all four lengths -- "an accumulator is never -0.0"."""
    _, d_pairs, m = special
    z = pairs_f32([-0.0] * N_SPECIAL, [-0.0] * N_SPECIAL)
    d_pairs.upload(z)
    jobs = [(first, n) for first in SPECIAL_FIRSTS for n in SPECIAL_LENGTHS]
    for lag in SPECIAL_LAGS:
        got = run_device(m, d_pairs, N_SPECIAL, jobs, lag, offset=0j)
        for k, (a, n) in enumerate(jobs):
            assert same_record_bits(got[k], special_sums(z[a:a + n], 0j, lag)), (lag, a, n, got[k])
            assert got[k].tobytes()[:64] == bytes(64) and (got[k]["n_pairs"], got[k]["n_lagged"]) == (n, max(n - lag, 0)), (lag, a, n, got[k])


def test_subnormals_and_flt_max_every_field_by_its_bits(special):
    """The buffer of tests/test_measure_host.py: multiples of the smallest f32 subnormal in front of pair 2 T + 150, +-FLT_MAX
    behind.  The terms are f64 conversions of the f32 values: a flushed subnormal gives a zero where the reference has 2^-149,
    an f32 product an infinity where it has 2^256."""
    _, d_pairs, m = special
    at = 2 * T + 150
    z = extremes_buffer(N_SPECIAL, at)
    d_pairs.upload(z)
    jobs = [(first, n) for first in SPECIAL_FIRSTS for n in SPECIAL_LENGTHS]
    jobs += [(at - 100, 257), (at + 1, T + 100), (at, 1), (at - 1, 2), (at - 1, 1), (3, N_SPECIAL - 3)]
    for lag in SPECIAL_LAGS:
        got = run_device(m, d_pairs, N_SPECIAL, jobs, lag, offset=0j)
        for k, (a, n) in enumerate(jobs):
            want = special_sums(z[a:a + n], 0j, lag)
            assert same_record(got[k], want) and same_record_bits(got[k], want), (lag, a, n, got[k], want)
            assert all(np.isfinite(got[k][f]) for f in M.NAMES + ("peak",)), (lag, a, n, got[k])
            if a + n <= at:
                assert got[k]["p"] > 0.0 and got[k]["q"] > 0.0 and got[k]["peak"] >= 2.0 ** -298, (lag, a, n, got[k])
        host = np.frombuffer(m.run(z, table(jobs), 0j, lag), dtype=M.SUMS)
        assert same_record_bits(host, got), lag


# ---- end to end: a recording with a constant-envelope burst and a noise-like one

N, ROWS, D, TAPS = R.N, 256, R.D, R.TAPS
FM_BURST = (30, 110, 200)          # first row, the row behind the last, the centre's bin from the middle
NOISE_BURST = (140, 230, -300)
RATE, FREQ = 8000000.0, 100.0


def bursts_recording():
    """int8 IQ: noise of sigma 20; an FM burst of amplitude 40, +-2 bins of deviation with a period of 8 rows; a burst of
    Gaussian noise of rms 30, 8 bins wide (white noise through a moving average of N / 8 samples)."""
    rng = np.random.default_rng(78)
    x = rng.normal(0.0, 20.0, N * ROWS) + 1j * rng.normal(0.0, 20.0, N * ROWS)
    t = np.arange(FM_BURST[0] * N, FM_BURST[1] * N)
    period = 8 * N
    x[t] += 40.0 * np.exp(1j * (2 * np.pi * (FM_BURST[2] / N) * t + (2.0 * period / N) * np.sin(2 * np.pi * t / period)))
    t = np.arange(NOISE_BURST[0] * N, NOISE_BURST[1] * N)
    white = rng.normal(0.0, 1.0, t.size + N // 8 - 1) + 1j * rng.normal(0.0, 1.0, t.size + N // 8 - 1)
    band = np.convolve(white, np.ones(N // 8), mode="valid")
    band *= 30.0 / np.sqrt(np.mean(np.abs(band) ** 2))
    x[t] += band * np.exp(2j * np.pi * (NOISE_BURST[2] / N) * t)
    raw = np.empty(2 * N * ROWS)
    raw[0::2], raw[1::2] = x.real, x.imag
    return np.clip(np.rint(raw), -128, 127).astype(np.int8).view(np.uint8)


def test_end_to_end_a_constant_envelope_and_a_noise_like_burst():
    raw = bursts_recording()
    c = fsea.lowpass_taps(RATE, 0.4 * RATE / D, TAPS)
    lead = fsea.extract_lead(TAPS, D)
    ejobs = []
    for b0, b1, k in (FM_BURST, NOISE_BURST):
        first = b0 * N + TAPS - 1 - lead + 5               # inside the burst from its first measured pair on, at an odd start
        ejobs.append(fsea.ExtractJob(first, (b1 * N - first) // D * D, first, -k / N, 0.0, 0))
    ex, m = fsea.Extract(c, D), fsea.Measure()
    laid, total = ex.layout(ejobs)
    d_iq, g_pairs = Guarded(raw.nbytes).upload(raw), Guarded(8 * total)
    ex.run_device(d_iq.addr, raw.size // 2, laid, g_pairs.addr, total, flip=True)
    mjobs = fsea.measure_jobs(laid, D, lead // D)
    assert [(j.first_pair, j.n_pairs) for j in mjobs] == [(e.out_first + lead // D, e.n_samples // D - lead // D) for e in laid]
    off = pedestal(c) * (1 + 1j)
    lag = 1
    got = run_device(m, g_pairs, total, [(j.first_pair, j.n_pairs) for j in mjobs], lag, offset=off)
    pairs = g_pairs.payload(np.complex64, (total,))
    g_pairs.check("the extract's output")
    results = []
    for k, j in enumerate(mjobs):
        assert same_record_bits(got[k], M.sums(pairs[j.first_pair:j.first_pair + j.n_pairs], off, lag)), k
        results.append(fsea.measure_finish(fsea.MeasureSums.from_buffer_copy(got[k].tobytes()), lag))
    fm, noise = results
    for name, r in (("fm", fm), ("noise", noise)):
        print(name, "power_db %.2f freq %.5f width %.5f kurtosis %.3f crest %.2f dc %.4f %.4f" %
              (r.power_db, r.freq_cycles, r.width_cycles, r.kurtosis, r.crest, r.dc_re, r.dc_im))
    assert fm.kurtosis < noise.kurtosis and fm.kurtosis < 1.5 < noise.kurtosis
    assert fm.width_cycles < noise.width_cycles
    # both were mixed to the centre of the decimated band, a sixteenth of a cycle per pair wide
    assert abs(fm.freq_cycles) < 0.02 and abs(noise.freq_cycles) < 0.02
    for o in (d_iq, g_pairs):
        o.free()
    for o in (ex, m):
        o.close()


def test_tool_measures_what_the_restatement_gives_for_its_files(tmp_path):
    raw = bursts_recording()
    raw.tofile(tmp_path / "bursts.raw")
    tool = os.path.join(BIN, "fsea-cutouts")
    common = [tool, str(tmp_path / "bursts.raw"), "--size", str(N), "--flip", "--offset", "60", "--min-rows", "8",
              "--gap-cols", "4", "--gap-rows", "2", "--decimation", str(D), "--rate", "8000000", "--freq", "100"]
    lag = 3
    plain = subprocess.run(common + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    with_m = subprocess.run(common + ["--out", str(tmp_path / "measured"), "--measures", "--lag", str(lag)], capture_output=True, text=True,
                            timeout=300)
    assert with_m.returncode == 0, with_m.stderr
    # everything but the new file is what it was, byte for byte
    assert with_m.stdout == plain.stdout and with_m.stderr == plain.stderr
    before, after = sorted(os.listdir(tmp_path / "plain")), sorted(os.listdir(tmp_path / "measured"))
    assert "measures.txt" not in before and after == sorted(before + ["measures.txt"])
    for name in before:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "measured" / name, "rb").read(), name
    files = [f for f in before if f.endswith(".cf32")]
    print(plain.stdout.strip(), files)
    assert len(files) == 2                                   # the two bursts, one event each
    off = pedestal(fsea.lowpass_taps(RATE, 0.4 * RATE / D, TAPS)) * (1 + 1j)
    lines = open(tmp_path / "measured" / "measures.txt").read().split("\n")
    assert lines[-1] == "" and len(lines) == len(files) + 1
    kurtosis = {}
    for line, name in zip(lines, files):
        y = np.fromfile(tmp_path / "measured" / name, dtype=np.complex64)
        r = fsea.measure_finish(fsea.MeasureSums.from_buffer_copy(M.sums(y, off, lag).tobytes()), lag)
        number = int(name[len("cutout-"):-len(".cf32")])
        want = "%d %d " % (number, y.size) + " ".join("%.9e" % v for v in (
            r.power_db, r.freq_cycles, r.freq_cycles * RATE / D / 1e6, r.width_cycles, r.kurtosis, r.crest, r.dc_re, r.dc_im))
        print(line)
        assert line == want, name
        kurtosis[number] = r.kurtosis
    # cutouts.txt says where each event lies: the longest one at the FM burst's columns against the longest at the noise burst's
    events = [e.split() for e in open(tmp_path / "measured" / "cutouts.txt").read().split("\n") if e]

    def longest_at(k):
        mine = [e for e in events if int(e[0]) in kurtosis and int(e[3]) - 8 <= N // 2 + k <= int(e[4]) + 8]
        assert mine, (k, events)
        return kurtosis[int(max(mine, key=lambda e: int(e[9]))[0])]

    assert longest_at(FM_BURST[2]) < longest_at(NOISE_BURST[2])
