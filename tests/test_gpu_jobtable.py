"""GPU tier: what fsea_extract and fsea_measure share (csrc/fsea_jobs.h) where it can go wrong -- the look-up of a workgroup's
job at the edges of the table, and the table's life across calls of different sizes on two streams.

Bit identity, no tolerance: every job of a table call equals the same job run alone in a one-job call, whose look-up takes
no step; one table per object is also held against the yardstick of its own tests (fsea.Zoom, tests/measure_ref.py).  The
shapes are the smallest at which the shared parts can still fail: tables of 1 (zero steps), 2, 3, 5, 64, 65 and 1025
entries, jobs without output in the first place, in the last and as two neighbours, every other job one tile of a few
outputs but for one of two tiles (129 outputs at D = 2; 4097 pairs); a recording of 11 KiB and a buffer of 57 KiB."""
import numpy as np
import pytest

from frequensea_amd import fsea
from tests import measure_ref as M
from tests.guarded import Guarded
from tests.test_gpu_extract import bits, zoom_pairs
from tests.test_gpu_measure import same_bits
from tests.test_gpu_zoom import lowpass_like_taps

pytestmark = pytest.mark.gpu

D, L = 2, 21
SIZES = (1, 2, 3, 5, 64, 65, 1025)
LIFE = (1, 300, 2, 1025, 1)              # the calls of one object, in this order, on two streams in turn
OFFSET, LAG = 0.5 + 0.5j, 1
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


class Shared:
    """one object of each kind, their inputs resident, and per table size what the one-job calls give: computed once"""

    def __init__(self):
        self.c = lowpass_like_taps(L, 31)
        self.ex, self.m = fsea.Extract(self.c, D), fsea.Measure()
        self.iq = np.random.default_rng(32).integers(0, 256, 2 * N_IQ, dtype=np.uint8)
        rng = np.random.default_rng(33)
        self.z = (rng.normal(0.0, 1.0, N_PAIRS) + 1j * rng.normal(0.0, 1.0, N_PAIRS) + OFFSET).astype(np.complex64)
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

    def close(self):
        for g in (self.d_iq, self.d_z):
            g.check("the input is read, not written")
            g.free()
        self.ex.close()
        self.m.close()


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
    assert same_bits(got, shared.measure_alone(n)), n
    assert got["n_pairs"].tolist() == [j.n_pairs for j in jobs]
    if n == 65:                            # and the jobs alone are the restatement's records
        for k, j in enumerate(jobs):
            want = M.sums(shared.z[j.first_pair:j.first_pair + j.n_pairs], OFFSET, LAG)
            assert same_bits(got[k], want), (k, j.first_pair, j.n_pairs)


def test_a_table_lives_across_calls_of_every_size_on_two_streams(shared):
    """One object of each kind, calls of 1, 300, 2, 1025 and 1 jobs on two streams in turn with no host wait between them:
    the mapped table and the device table grow twice and are used again for less, each call's fill waits for the upload
    of the one before (`copied`), each call's kernels for the previous user of the device table (the scratch's event)."""
    references = [(shared.extract_alone(n), shared.measure_alone(n)) for n in LIFE]
    ex, m, sync = fsea.Extract(shared.c, D), fsea.Measure(), fsea.Plan(128)
    streams = (fsea.Stream(), fsea.Stream())
    tables = [ex.layout(extract_jobs(n)) for n in LIFE]
    outputs = [(Guarded(8 * total), total, Guarded(80 * n)) for (_, total), n in zip(tables, LIFE)]     # allocated before the first call
    for k, ((table, total), (g_pairs, _, g_sums), n) in enumerate(zip(tables, outputs, LIFE)):
        ex.run_device(shared.d_iq.addr, N_IQ, table, g_pairs.addr, total, flip=True, stream=streams[k % 2])
        m.run_device(shared.d_z.addr, N_PAIRS, measure_jobs(n), g_sums.addr, offset=OFFSET, lag=LAG, stream=streams[(k + 1) % 2])
    for s in streams:                      # the one wait, at the end
        sync.synchronize(s)
    for (g_pairs, total, g_sums), (want_pairs, want_sums), n in zip(outputs, references, LIFE):
        assert np.array_equal(finish(g_pairs, np.uint32, (total, 2), "extract, call of %d" % n), want_pairs), n
        assert same_bits(finish(g_sums, M.SUMS, (n,), "measure, call of %d" % n), want_sums), n
    for o in streams + (sync, ex, m):
        o.close()
