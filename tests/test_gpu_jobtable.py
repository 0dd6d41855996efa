"""GPU tier: what fsea_extract, fsea_measure, fsea_audio and fsea_spectra share (csrc/fsea_jobs.h) where it can go wrong -- the
look-up of a workgroup's job at the edges of the table, the table's life across calls of different sizes on two streams, and
the host form of the three objects that place their outputs, on a table with gaps.

Bit identity, no tolerance: every job of a table call equals the same job run alone in a one-job call, whose look-up takes
no step; one table per object is also held against the yardstick of its own tests (fsea.Zoom, tests/measure_ref.py,
tests/audio_ref.py; tests/spectra_ref.py within the bound of tests/test_gpu_spectra.py).  The shapes are the smallest at
which the shared parts can still fail: tables of 1 (zero steps), 2, 3, 5, 64, 65 and 1025 entries, jobs without output in the
first place, in the last and as two neighbours, every other job one tile of a few outputs but for one of two tiles (129
outputs at D = 2; 4097 pairs; 257 audio outputs at D2 = 2 and 21 taps, whose tile is 256; 33 segments of 64 pairs every 32,
whose tile is 32); a recording of 11 KiB and a buffer of 57 KiB."""
import ctypes

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import audio_ref as A
from tests import measure_ref as M
from tests import spectra_ref as S
from tests.guarded import Guarded
from tests.jobs_common import pairs_of, same_float_bits, same_record_bits
from tests.test_gpu_audio import taps_of
from tests.test_gpu_extract import bits, zoom_pairs
from tests.test_gpu_spectra import worst_over_bound
from tests.test_gpu_zoom import lowpass_like_taps

pytestmark = pytest.mark.gpu

D, L = 2, 21
SIZES = (1, 2, 3, 5, 64, 65, 1025)
LIFE = (1, 300, 2, 1025, 1)              # the calls of one object, in this order, on two streams in turn
OFFSET, LAG = 0.5 + 0.5j, 1
D2, L2, GAIN = 2, 21, 0.75               # the audio object: FM, a tile of 256 outputs
AUDIO_TILE = 256
SP_N, SP_HOP = 64, 32                    # the spectra object: "z" under a Hann taper, a tile of 32 segments
N_IQ = 5 * 1025 + 2 * (fsea.ZOOM_TILE_OUTPUTS + 1) + 8
N_PAIRS = 3 * 1025 + fsea.MEASURE_TILE_PAIRS + 8


def kinds(n):
    """what each of the n places of a table holds: "empty" in the first, the last and two neighbouring places as far as n has
    them, "two" (tiles) in one place, "one" in the others"""
    two = 0 if n == 1 else 1 if n <= 5 else n // 3
    empty = ({0, n - 1, n // 2, n // 2 + 1} & set(range(n))) - {two}
    return ["two" if i == two else "empty" if i in empty else "one" for i in range(n)]


def test_the_tables_have_the_edges_they_are_for():
    assert kinds(1) == ["two"] and kinds(2) == ["empty", "two"] and kinds(3) == ["empty", "two", "empty"]
    assert kinds(5) == ["empty", "two", "empty", "empty", "empty"]
    for n in (64, 65, 300, 1025):
        k = kinds(n)
        assert k[0] == k[-1] == k[n // 2] == k[n // 2 + 1] == "empty" and k.count("empty") == 4 and k.count("two") == 1


def extract_jobs(n):
    """n jobs, each with its own first (every residue mod 8), centre and stream position; an empty one has fewer than D samples"""
    samples = {"empty": lambda i: i % D, "one": lambda i: D * (1 + i % 5) + i % D, "two": lambda i: D * (fsea.ZOOM_TILE_OUTPUTS + 1)}
    return [fsea.ExtractJob(5 * i + i % 3, samples[k](i), 77 + 9 * i, ((i * 37) % 201 - 100) / 256.0, 0.25 * (i % 4), 0)
            for i, k in enumerate(kinds(n))]


def measure_jobs(n):
    """n spans at even and odd first pairs"""
    pairs = {"empty": lambda i: 0, "one": lambda i: 1 + i % 7, "two": lambda i: fsea.MEASURE_TILE_PAIRS + 1}
    return (fsea.MeasureJob * n)(*[fsea.MeasureJob(3 * i + i % 2, pairs[k](i)) for i, k in enumerate(kinds(n))])


def audio_jobs(n):
    """n spans at even and odd first pairs; an empty one has fewer than D2 pairs"""
    pairs = {"empty": lambda i: i % D2, "one": lambda i: D2 * (1 + i % 5) + i % D2, "two": lambda i: D2 * (AUDIO_TILE + 1)}
    return [fsea.AudioJob(3 * i, pairs[k](i), 0) for i, k in enumerate(kinds(n))]


def spectra_jobs(n):
    """n spans at even and odd first pairs; an empty one has fewer than SP_N pairs"""
    pairs = {"empty": lambda i: i % SP_N, "one": lambda i: SP_N + SP_HOP * (i % 3) + i % 7,
             "two": lambda i: SP_N + SP_HOP * fsea.SPECTRA_TILE_SEGMENTS + 5}
    return [fsea.SpectraJob(3 * i, pairs[k](i), 0) for i, k in enumerate(kinds(n))]


def test_the_spectra_tables_have_one_job_past_the_tile():
    assert fsea.SPECTRA_TILE_SEGMENTS == S.TILE_SEGMENTS == 32
    for n, empty in zip(sorted(set(SIZES + LIFE)), (0, 1, 2, 4, 4, 4, 4, 4)):
        segments = [S.segments(j.n_pairs, SP_N, SP_HOP) for j in spectra_jobs(n)]
        assert segments.count(33) == 1 and segments.count(0) == empty and set(segments) <= {0, 1, 2, 3, 33}, n
        assert all(j.first_pair + j.n_pairs <= N_PAIRS for j in spectra_jobs(n)), n
        if n == 1025:
            assert sum(-(-s // S.TILE_SEGMENTS) for s in segments) == 1022


class Shared:
    """one object of each kind, their inputs resident, and per table size what the one-job calls give: computed once"""

    def __init__(self):
        self.c = lowpass_like_taps(L, 31)
        self.c2 = taps_of(L2)
        self.ex, self.m, self.au = fsea.Extract(self.c, D), fsea.Measure(), fsea.Audio("fm", self.c2, D2)
        self.w = fsea.window("hann", SP_N)
        self.sp = fsea.Spectra(SP_N, SP_HOP, "z", self.w)
        self.iq = np.random.default_rng(32).integers(0, 256, 2 * N_IQ, dtype=np.uint8)
        self.z = pairs_of(33, N_PAIRS)
        self.d_iq, self.d_z = Guarded(self.iq.nbytes).upload(self.iq), Guarded(self.z.nbytes).upload(self.z)
        self.alone = {}

    def extract_table(self, n):
        return self.ex.layout(extract_jobs(n))

    def extract_alone(self, n):
        """the pairs buffer of the table of n jobs as n one-job calls fill it, each at its own out_first"""
        if ("extract", n) not in self.alone:
            table, total = self.extract_table(n)
            g = Guarded(8 * total)
            for j in table:
                self.ex.run_device(self.d_iq.addr, N_IQ, [j], g.addr, total, flip=True)
            self.alone["extract", n] = finish(g, np.uint32, (total, 2), "extract, %d one-job calls" % n)
        return self.alone["extract", n]

    def measure_alone(self, n):
        """the records of the table of n jobs as n one-job calls write them, each to its own place"""
        if ("measure", n) not in self.alone:
            jobs = measure_jobs(n)
            g = Guarded(80 * n)
            for k, j in enumerate(jobs):
                self.m.run_device(self.d_z.addr, N_PAIRS, [j], g.addr + 80 * k, offset=OFFSET, lag=LAG)
            self.alone["measure", n] = finish(g, M.SUMS, (n,), "measure, %d one-job calls" % n)
        return self.alone["measure", n]

    def audio_table(self, n):
        return self.au.layout(audio_jobs(n))

    def audio_alone(self, n):
        """the audio buffer of the table of n jobs as n one-job calls fill it, each at its own out_first"""
        if ("audio", n) not in self.alone:
            table, total = self.audio_table(n)
            g = Guarded(4 * total)
            for j in table:
                self.au.run_device(self.d_z.addr, N_PAIRS, [j], g.addr, total, offset=OFFSET, gain=GAIN)
            self.alone["audio", n] = finish(g, np.uint32, (total,), "audio, %d one-job calls" % n)
        return self.alone["audio", n]

    def spectra_table(self, n):
        return self.sp.layout(spectra_jobs(n))

    def spectra_alone(self, n):
        """the power buffer of the table of n jobs as n one-job calls fill it, each at its own out_first"""
        if ("spectra", n) not in self.alone:
            table, total = self.spectra_table(n)
            g = Guarded(4 * total)
            for j in table:
                self.sp.run_device(self.d_z.addr, N_PAIRS, [j], g.addr, total, offset=OFFSET)
            self.alone["spectra", n] = finish(g, np.uint32, (total,), "spectra, %d one-job calls" % n)
        return self.alone["spectra", n]

    def close(self):
        for g in (self.d_iq, self.d_z):
            g.check("the input is read, not written")
            g.free()
        for o in (self.ex, self.m, self.au, self.sp):
            o.close()


def finish(g, dtype, shape, what):
    """a guarded output's payload, its bands checked, the buffer freed (the download waits for the null stream)"""
    got = g.payload(dtype, shape)
    g.check(what)
    g.free()
    return got


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.close()


@pytest.mark.parametrize("n", SIZES)
def test_extract_finds_every_job_of_a_table(shared, n):
    table, total = shared.extract_table(n)
    assert sum(1 for j in table if j.n_samples // D == fsea.ZOOM_TILE_OUTPUTS + 1) == 1
    assert all(j.first + j.n_samples <= N_IQ for j in table) and (n < 64 or {j.first % 8 for j in table} == set(range(8)))
    g = Guarded(8 * total)
    shared.ex.run_device(shared.d_iq.addr, N_IQ, table, g.addr, total, flip=True)
    got = finish(g, np.uint32, (total, 2), "extract, a table of %d" % n)
    assert np.array_equal(got, shared.extract_alone(n)), n
    if n == 65:                            # and the jobs alone are the zoom's pairs, as tests/test_gpu_extract.py has it
        zoom = fsea.Zoom(shared.c, D, 128)
        for i, j in enumerate(table):
            want = zoom_pairs(zoom, shared.iq, j, 1)
            assert want.size == j.n_samples // D
            assert np.array_equal(got[j.out_first:j.out_first + want.size].ravel(), bits(want).ravel()), i
        zoom.close()


@pytest.mark.parametrize("n", SIZES)
def test_measure_finds_every_job_of_a_table(shared, n):
    jobs = measure_jobs(n)
    assert sum(1 for j in jobs if j.n_pairs == fsea.MEASURE_TILE_PAIRS + 1) == 1
    assert all(j.first_pair + j.n_pairs <= N_PAIRS for j in jobs)
    g = Guarded(80 * n)
    shared.m.run_device(shared.d_z.addr, N_PAIRS, jobs, g.addr, offset=OFFSET, lag=LAG)
    got = finish(g, M.SUMS, (n,), "measure, a table of %d" % n)
    assert same_record_bits(got, shared.measure_alone(n)), n
    assert got["n_pairs"].tolist() == [j.n_pairs for j in jobs]
    if n == 65:                            # and the jobs alone are the restatement's records
        for k, j in enumerate(jobs):
            want = M.sums(shared.z[j.first_pair:j.first_pair + j.n_pairs], OFFSET, LAG)
            assert same_record_bits(got[k], want), (k, j.first_pair, j.n_pairs)


@pytest.mark.parametrize("n", SIZES)
def test_audio_finds_every_job_of_a_table(shared, n):
    assert A.tile(D2, L2) == AUDIO_TILE
    table, total = shared.audio_table(n)
    assert sum(1 for j in table if j.n_pairs // D2 == AUDIO_TILE + 1) == 1 and total == sum(j.n_pairs // D2 for j in table)
    assert all(j.first_pair + j.n_pairs <= N_PAIRS for j in table) and (n < 2 or {j.first_pair % 2 for j in table} == {0, 1})
    g = Guarded(4 * total)
    shared.au.run_device(shared.d_z.addr, N_PAIRS, table, g.addr, total, offset=OFFSET, gain=GAIN)
    got = finish(g, np.uint32, (total,), "audio, a table of %d" % n)
    assert np.array_equal(got, shared.audio_alone(n)), n
    if n == 65:                            # and the jobs alone are the restatement's audio
        for k, j in enumerate(table):
            want = A.audio(shared.z[j.first_pair:j.first_pair + j.n_pairs], A.FM, shared.c2, D2, OFFSET, GAIN)
            assert want.size == j.n_pairs // D2
            assert same_float_bits(got[j.out_first:j.out_first + want.size].view(np.float32), want), (k, j.first_pair, j.n_pairs)


@pytest.mark.parametrize("n", SIZES)
def test_spectra_finds_every_job_of_a_table(shared, n):
    table, total = shared.spectra_table(n)
    counts = [SP_N if S.segments(j.n_pairs, SP_N, SP_HOP) else 0 for j in table]
    assert total == sum(counts) and (n < 2 or {j.first_pair % 2 for j in table} == {0, 1})
    g = Guarded(4 * total)
    shared.sp.run_device(shared.d_z.addr, N_PAIRS, table, g.addr, total, offset=OFFSET)
    got = finish(g, np.uint32, (total,), "spectra, a table of %d" % n)
    assert np.array_equal(got, shared.spectra_alone(n)), n
    if n == 65:                            # and the jobs alone lie within the bound of the restatement
        for k, (j, count) in enumerate(zip(table, counts)):
            power = got[j.out_first:j.out_first + count].view(np.float32)
            over = worst_over_bound(power, shared.z[j.first_pair:j.first_pair + j.n_pairs], shared.sp, shared.w)
            assert over <= 1.0, (k, j.first_pair, j.n_pairs, over)


SENTINEL = 0xFFC12345                    # a NaN no kernel here computes


@pytest.mark.parametrize("kind", ["extract", "audio", "spectra"])
def test_the_host_form_hands_back_the_jobs_own_ranges_and_nothing_else(shared, kind):
    """fsea_extract_run_host, fsea_audio_run_host and fsea_spectra_run_host on a table laid out by hand: out_first neither back to back nor ascending,
    the middle job without output and its out_first inside the first job's range.  Each job's range is what the binding's
    run() returns for it (its own layout, back to back); every other element of the caller's array keeps its bits."""
    L_ = fsea.hip_lib()
    if kind == "extract":
        jobs = [fsea.ExtractJob(9, D * 40, 500, 0.11, 0.25, 100), fsea.ExtractJob(3, 1, 77, -0.2, 0.0, 110),
                fsea.ExtractJob(130, D * 33 + 1, 9, -0.3, 0.5, 10)]
        counts, capacity, width = [j.n_samples // D for j in jobs], 160, 2
        want = shared.ex.run(shared.iq, jobs, flip=True)
        out = np.full(capacity * width, SENTINEL, np.uint32)
        table = (fsea.ExtractJob * 3)(*jobs)
        rc = L_.fsea_extract_run_host(shared.ex._p, shared.iq.ctypes.data, N_IQ, 1, ctypes.addressof(table), 3, out.ctypes.data, capacity)
    elif kind == "audio":
        jobs = [fsea.AudioJob(5, D2 * 37 + 1, 90), fsea.AudioJob(0, 1, 95), fsea.AudioJob(12, D2 * 29, 7)]
        counts, capacity, width = [j.n_pairs // D2 for j in jobs], 150, 1
        want = shared.au.run(shared.z, jobs, OFFSET, GAIN)
        out = np.full(capacity * width, SENTINEL, np.uint32)
        table = (fsea.AudioJob * 3)(*jobs)
        rc = L_.fsea_audio_run_host(shared.au._p, shared.z.ctypes.data, N_PAIRS, ctypes.addressof(table), 3, OFFSET.real, OFFSET.imag,
                                    GAIN, out.ctypes.data, capacity)
    else:
        jobs = [fsea.SpectraJob(5, SP_N + 2 * SP_HOP + 1, 90), fsea.SpectraJob(0, SP_N - 1, 100), fsea.SpectraJob(12, SP_N, 7)]
        counts, capacity, width = [SP_N if S.segments(j.n_pairs, SP_N, SP_HOP) else 0 for j in jobs], 160, 1
        want = shared.sp.run(shared.z, jobs, OFFSET)
        out = np.full(capacity * width, SENTINEL, np.uint32)
        table = (fsea.SpectraJob * 3)(*jobs)
        rc = L_.fsea_spectra_run_host(shared.sp._p, shared.z.ctypes.data, N_PAIRS, ctypes.addressof(table), 3, OFFSET.real, OFFSET.imag,
                                      out.ctypes.data, capacity)
    assert rc == 0, L_.fsea_last_error_string()
    assert counts[1] == 0 and counts[0] > 24 and counts[2] > 24
    firsts = [j.out_first for j in jobs]
    assert firsts[0] > firsts[2] + counts[2] and firsts[0] < firsts[1] < firsts[0] + counts[0]
    own = np.zeros(capacity * width, bool)
    for j, n, w in zip(jobs, counts, want):
        assert w.size == n
        own[width * j.out_first:width * (j.out_first + n)] = True
        assert np.array_equal(out[width * j.out_first:width * (j.out_first + n)], np.ascontiguousarray(w).view(np.uint32)), j.out_first
    assert own.sum() == width * sum(counts) and np.all(out[~own] == SENTINEL)
    assert not np.any(out[own] == SENTINEL)


def test_a_table_lives_across_calls_of_every_size_on_two_streams(shared):
    """One object of each kind, calls of 1, 300, 2, 1025 and 1 jobs on two streams in turn with no host wait between them:
    the mapped table and the device table grow twice and are used again for less, each call's fill waits for the upload
    of the one before (`copied`), each call's kernels for the previous user of the device table (the scratch's event)."""
    references = [(shared.extract_alone(n), shared.measure_alone(n), shared.audio_alone(n), shared.spectra_alone(n)) for n in LIFE]
    ex, m, au, sync = fsea.Extract(shared.c, D), fsea.Measure(), fsea.Audio("fm", shared.c2, D2), fsea.Plan(128)
    sp = fsea.Spectra(SP_N, SP_HOP, "z", shared.w)
    streams = (fsea.Stream(), fsea.Stream())
    tables = [(ex.layout(extract_jobs(n)), au.layout(audio_jobs(n)), sp.layout(spectra_jobs(n))) for n in LIFE]
    outputs = [(Guarded(8 * total), total, Guarded(80 * n), Guarded(4 * floats), floats, Guarded(4 * powers), powers)
               for ((_, total), (_, floats), (_, powers)), n in zip(tables, LIFE)]                      # allocated before the first call
    for k, (((table, total), (spans, floats), (cuts, powers)), (g_pairs, _, g_sums, g_audio, _, g_power, _), n) in enumerate(
            zip(tables, outputs, LIFE)):
        ex.run_device(shared.d_iq.addr, N_IQ, table, g_pairs.addr, total, flip=True, stream=streams[k % 2])
        m.run_device(shared.d_z.addr, N_PAIRS, measure_jobs(n), g_sums.addr, offset=OFFSET, lag=LAG, stream=streams[(k + 1) % 2])
        au.run_device(shared.d_z.addr, N_PAIRS, spans, g_audio.addr, floats, offset=OFFSET, gain=GAIN, stream=streams[k % 2])
        sp.run_device(shared.d_z.addr, N_PAIRS, cuts, g_power.addr, powers, offset=OFFSET, stream=streams[(k + 1) % 2])
    for s in streams:                      # the one wait, at the end
        sync.synchronize(s)
    for (g_pairs, total, g_sums, g_audio, floats, g_power, powers), (want_pairs, want_sums, want_audio, want_power), n in zip(
            outputs, references, LIFE):
        assert np.array_equal(finish(g_pairs, np.uint32, (total, 2), "extract, call of %d" % n), want_pairs), n
        assert same_record_bits(finish(g_sums, M.SUMS, (n,), "measure, call of %d" % n), want_sums), n
        assert np.array_equal(finish(g_audio, np.uint32, (floats,), "audio, call of %d" % n), want_audio), n
        assert np.array_equal(finish(g_power, np.uint32, (powers,), "spectra, call of %d" % n), want_power), n
    for o in streams + (sync, ex, m, au, sp):
        o.close()
