"""GPU tier: cut-out spectra (fsea_spectra_*, kernels fsea_spectra_tiles_<n> and fsea_spectra_fold) and fsea-cutouts --spectra.

Parity: a job's n powers against tests/spectra_ref.py -- the terms, kinds, taper and sign in f32 as the header words them,
an exact-to-f64 transform, the average in f64 -- per bin within 2 PER_BIN_TOL (1 + 1e-6) mean_s(max_k p_s[k]) + 1e-6: the
FFT paths' per-bin bound carried through the square.  A correct f32 transform uses a few hundredths of that, so the bound
alone would hide a small mistake; the structural tests are where a kernel goes wrong: a job's bits alone, repeated, among
hundreds of others and at either parity of first_pair; the lengths round one segment; the tile seam on inputs whose
segments are all the same, where any S must give the bits of S = 1; a taper of ones; a NaN pair; the host form; two
streams; refusals.  Every one of the seven sizes runs in the parity, in both seam tests and in the closed forms: the radix-2
pass is the only path of n = 128, 512, 2048, and 1024 is where a round becomes one segment.  Small shapes, but for the one
job of FSEA_SPECTRA_MAX_PAIRS.  Inputs and outputs are guarded."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import extract_ref as X
from tests import spectra_ref as R
from tests.conftest import ROOT
from tests.guarded import FILL, Guarded
from tests.jobs_common import address, same_float_bits
from tests.jobs_common import run_device as run_placed
from tests.parity import PER_BIN_TOL

pytestmark = pytest.mark.gpu

OFFSET = 0.5 + 0.5j
BIN = os.path.join(ROOT, "frequensea_amd", "bin")
FSEA_EINVAL = -1
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
SEGMENTS = 7                      # of a parity job
SIGNAL_PAIRS = 4096 + (SEGMENTS - 1) * 4096 + 2
POWER_TOL = 2.0 * PER_BIN_TOL * (1.0 + 1e-6)      # 4.000004e-6: if each segment's magnitude is within PER_BIN_TOL of its largest ...


def bound(scale):
    return POWER_TOL * scale + 1e-6


def hops(n):
    return [n, n // 2, n // 4 + 3] + ([1] if n in (64, 128) else [])      # 128: the smallest size with the radix-2 pass


def laid_out(obj, jobs, gap=3):
    """the (first_pair, n_pairs) as a table with their outputs in table order, `gap` floats of fill between them; the floats"""
    at, rows = gap, []
    for a, m in jobs:
        rows.append(fsea.SpectraJob(a, m, at))
        at += (obj.n if R.segments(m, obj.n, obj.hop) else 0) + gap
    return (fsea.SpectraJob * len(rows))(*rows), at


def run_device(obj, d_pairs, n_buffer, table, n_power, offset=OFFSET, stream=0, wait=None):
    """one call into a guarded output pre-filled with FILL -> one float32 array per job; no float outside the jobs' is written"""
    return run_placed(obj, d_pairs, n_buffer, table, n_power, lambda j: obj.n if R.segments(j.n_pairs, obj.n, obj.hop) else 0,
                      "powers", stream, wait, offset=offset)


def worst_over_bound(got, pairs, obj, window):
    want, scale = R.spectrum(pairs, obj.n, obj.hop, obj.kind, window, OFFSET)
    assert got.shape == want.shape
    if want.size == 0:
        return 0.0
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got.astype(np.float64) - want))) / bound(scale)


# ---- parity ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cutouts():
    """the QPSK-plus-noise cut-out and the noise-alone one behind one another, resident"""
    m = SIGNAL_PAIRS
    z = np.concatenate([R.qpsk_cutout(m), R.noise_cutout(m)])
    d = Guarded(z.nbytes).upload(z)
    yield z, d
    d.check("the input is read, not written")
    d.free()


@pytest.mark.parametrize("window", ["rect", "hann"])
@pytest.mark.parametrize("n", SIZES)
def test_every_bin_lies_within_the_bound_of_the_restatement(cutouts, n, window):
    z, d_pairs = cutouts
    w = None if window == "rect" else fsea.window("hann", n)
    if w is not None:
        assert np.array_equal(w, R.hann(n)) or np.max(np.abs(w - R.hann(n))) <= 2.0 ** -23
    worst = 0.0
    for kind in R.KINDS:
        for hop in hops(n):
            obj = fsea.Spectra(n, hop, kind, w)
            m = n + (SEGMENTS - 1) * hop
            assert obj.segments(m) == SEGMENTS and m + 1 <= SIGNAL_PAIRS
            jobs = [(1, m), (SIGNAL_PAIRS + 2, m)]              # the emission at an odd first, the noise at an even one
            table, n_power = laid_out(obj, jobs)
            got = run_device(obj, d_pairs, z.size, table, n_power)
            for (a, _), g in zip(jobs, got):
                over = worst_over_bound(g, z[a:a + m], obj, w)
                print("n", n, window, "kind", kind, "hop", hop, "first", a, "worst error over the bound: %.4f" % over)
                worst = max(worst, over)
            obj.close()
    print("n", n, window, "worst of all kinds and hops: %.4f" % worst)
    assert worst <= 1.0


# ---- structure ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,hop", [(256, 77), (128, 45)])
def test_the_table_does_not_change_a_bit(cutouts, n, hop):
    """The same spans alone, twice in one table, among 300 mixed-length jobs in a shuffled order, and the same pairs at an odd
    and at an even first_pair: identical bits per job.  At 128 a round is eight segments and ends in the radix-2 pass."""
    z, _ = cutouts
    data = z[5:5 + 3000]
    buf = np.concatenate([data, z[:1], data])                      # the same pairs from pair 0 and from pair 3001
    d = Guarded(buf.nbytes).upload(buf)
    obj = fsea.Spectra(n, hop, "fourth", fsea.window("hann", n))
    lengths = [n, n + hop, 1000, 2999, 3000, 32 * hop + n, 33 * hop + n]
    alone = {}
    for m in lengths:
        for first in (0, 3001):
            table, n_power = laid_out(obj, [(first, m)], gap=0)
            alone[(first, m)] = run_device(obj, d, buf.size, table, n_power)[0]
        assert same_float_bits(alone[(0, m)], alone[(3001, m)]), m        # either parity
        assert worst_over_bound(alone[(0, m)], data[:m], obj, fsea.window("hann", n)) <= 1.0
    rng = np.random.default_rng(12)
    jobs = [(int(rng.integers(0, 3000)), int(rng.integers(0, 2900))) for _ in range(300)]
    jobs = [(a, min(m, buf.size - a)) for a, m in jobs]
    special = [(first, m) for m in lengths for first in (0, 3001)] * 2       # every one twice
    jobs += special
    order = rng.permutation(len(jobs))
    shuffled = [jobs[k] for k in order]
    table, n_power = laid_out(obj, shuffled, gap=1)
    got = run_device(obj, d, buf.size, table, n_power)
    seen = 0
    for at, k in enumerate(order):
        a, m = jobs[k]
        if (a, m) in alone:
            assert same_float_bits(got[at], alone[(a, m)]), (a, m)
            seen += 1
        elif at % 10 == 0:                                          # and the others are right too
            assert got[at].size == (n if m >= n else 0)
            assert worst_over_bound(got[at], buf[a:a + m], obj, fsea.window("hann", n)) <= 1.0
    assert seen >= len(special)
    d.check("the input is read, not written")
    d.free()
    obj.close()


@pytest.mark.parametrize("n,hop", [(64, 1), (64, 37), (256, 128), (4096, 4096), (4096, 1001), (128, 1), (512, 511), (1024, 1024), (2048, 3)])
def test_the_lengths_round_one_segment(cutouts, n, hop):
    z, d_pairs = cutouts
    obj = fsea.Spectra(n, hop, "sq")
    ns = [0, n - 1, n, n + hop - 1, n + hop]
    assert [obj.segments(m) for m in ns] == [0, 0, 1, 1, 2] == [R.segments(m, n, hop) for m in ns]
    table, n_power = laid_out(obj, [(3, m) for m in ns])
    got = run_device(obj, d_pairs, z.size, table, n_power)          # run_device: the floats of no job keep their fill
    assert [g.size for g in got] == [0, 0, n, n, n]
    assert same_float_bits(got[2], got[3])                                # the pairs behind the last whole segment are not read
    for m, g in zip(ns, got):
        assert worst_over_bound(g, z[3:3 + m], obj, None) <= 1.0
    assert not same_float_bits(got[3], got[4])
    obj.close()


@pytest.mark.parametrize("n,hop", [(64, 16), (256, 3), (4096, 2048), (128, 24), (512, 7), (1024, 512), (2048, 100)])
def test_the_tile_seam(n, hop):
    """Pairs with the period of the hop: every segment is the same, its power p an f32, and S p is exact in f64 for any S
    here -- so the average is p itself, bit for bit, for every S: one short of a tile, a tile, one more, two tiles and one.
    A segment that is left out or counted twice at a seam shows as (S - 1) / S or (S + 1) / S of it."""
    T = fsea.SPECTRA_TILE_SEGMENTS
    counts = [1, T - 1, T, T + 1, 2 * T + 1]
    base = R.noise_cutout(hop, seed=40 + n)
    total = n + 2 * T * hop
    z = np.tile(base, -(-total // hop) + 1)[:total + 1]
    d = Guarded(z.nbytes).upload(z)
    w = fsea.window("hann", n)
    for kind in ("z", "fourth"):
        obj = fsea.Spectra(n, hop, kind, w)
        jobs = [(0, n + (S - 1) * hop) for S in counts]
        assert [obj.segments(m) for _, m in jobs] == counts
        table, n_power = laid_out(obj, jobs)
        got = run_device(obj, d, z.size, table, n_power)
        assert worst_over_bound(got[0], z[:n], obj, w) <= 1.0 and np.all(got[0] >= 0)
        for S, g in zip(counts, got):
            assert same_float_bits(g, got[0]), (kind, S)
        # and on pairs that do differ from segment to segment the seam keeps the bound
        obj.close()
    d.check("the input is read, not written")
    d.free()


@pytest.mark.parametrize("n", SIZES)
def test_the_tile_seam_on_segments_that_differ(cutouts, n):
    """A round is G = max(1, 1024 / n) segments, a tile T = 32 of them: 2, 4, 8, 16 or 32 rounds.  Jobs that end one short of
    a round, with it, one behind it, behind the second, and the same round a tile, in one table at an odd first_pair, on
    segments that differ: a segment dropped, doubled or read from a neighbour's place in the LDS image moves a bin by
    percent of the scale, and the bound is 4e-6 of it."""
    z, d_pairs = cutouts
    T = fsea.SPECTRA_TILE_SEGMENTS
    G = max(1, 1024 // n)
    counts = sorted({S for S in (1, G - 1, G, G + 1, 2 * G + 1, T - 1, T, T + 1) if S > 0})
    hop = 5 if n <= 512 else 37
    obj = fsea.Spectra(n, hop, "fourth" if (n.bit_length() - 1) % 2 else "env")
    jobs = [(3, n + (S - 1) * hop) for S in counts]
    assert [obj.segments(m) for _, m in jobs] == counts and 3 + n + T * hop <= SIGNAL_PAIRS
    table, n_power = laid_out(obj, jobs)
    got = run_device(obj, d_pairs, z.size, table, n_power)
    for S, (a, m), g in zip(counts, jobs, got):
        over = worst_over_bound(g, z[a:a + m], obj, None)
        print("n", n, "G", G, "S", S, "worst error over the bound: %.4f" % over)
        assert over <= 1.0, (n, S)
    obj.close()


def test_the_longest_job_the_checks_accept():
    """One buffer of FSEA_SPECTRA_MAX_PAIRS pairs with the period of the hop, so every segment has the same f32 power p and
    S p is exact in f64 (S < 2^29): the one-segment job, the job of all 2^24 pairs and the one that begins a hop later and
    ends with the buffer have the same bits -- at (64, 16) through 1,048,573 segments in 32,768 tiles, sixteen segments a
    round; at (2048, 2048) through 8,192 segments in 256 tiles, a segment a round and the radix-2 pass.  The segment and
    tile arithmetic of the kernel and the fold's loop run at the largest counts the checks let through; one pair more is
    refused."""
    M = fsea.SPECTRA_MAX_PAIRS
    assert M == 1 << 24
    d = Guarded(8 * M)
    L_ = fsea.hip_lib()
    for n, hop, segments, tiles in ((64, 16, 1048573, 32768), (2048, 2048, 8192, 256)):
        z = np.tile(R.noise_cutout(hop, seed=60 + n), M // hop)
        assert z.size == M
        d.upload(z)
        w = fsea.window("hann", n)
        obj = fsea.Spectra(n, hop, "z", w)
        assert obj.segments(M) == R.segments(M, n, hop) == segments and -(-segments // fsea.SPECTRA_TILE_SEGMENTS) == tiles
        jobs = [(0, n), (0, M), (hop, M - hop)]
        assert obj.segments(M - hop) == R.segments(M - hop, n, hop) == segments - 1
        table, n_power = laid_out(obj, jobs)
        got = run_device(obj, d, M, table, n_power)
        over = worst_over_bound(got[0], z[:n], obj, w)
        print("n", n, "hop", hop, "S = 1, worst error over the bound: %.4f" % over)
        assert over <= 1.0 and np.all(got[0] >= 0)
        assert same_float_bits(got[1], got[0]), (n, "all of the buffer")
        assert same_float_bits(got[2], got[0]), (n, "to the end of the buffer")
        # one pair more than the longest: refused by name, in a buffer that is too short for it and in one that is not (the
        # pair behind the payload is the guard band's, allocated), and no float is written
        g = Guarded(4 * n_power)
        for n_buffer, word in ((M, b"job 1: pairs 0 .. 0 + 16777217 lie past"), (M + 1, b"job 1: n_pairs 16777217 too large")):
            tab = (fsea.SpectraJob * 2)(fsea.SpectraJob(0, n, 0), fsea.SpectraJob(0, M + 1, n))
            rc = L_.fsea_spectra_run_device(obj._p, d.addr, n_buffer, address(tab), 2, OFFSET.real, OFFSET.imag, g.addr, n_power, None)
            assert rc == FSEA_EINVAL and word in L_.fsea_last_error_string(), (rc, L_.fsea_last_error_string())
        assert np.all(g.payload(np.uint8, (4 * n_power,)) == FILL)
        g.check("a refused call")
        g.free()
        obj.close()
    d.check("the input is read, not written")
    d.free()


@pytest.mark.parametrize("n", SIZES)
def test_constant_pairs_and_an_impulse_give_their_closed_forms_bit_for_bit(n):
    """Constant pairs: (-1)^j puts all of a segment in bin n / 2; pass 0 adds four equal values and from there on every
    non-zero value meets the twiddle 1 alone, so bin n / 2 is n^2 (u u + v v) in f32 and every other bin +0, for each kind.
    One impulse in pair 0: pass 0 copies it to four places, every later butterfly adds zeros to it, and each of the n bins is
    |4 - 2i|^2 = 20.  A bin that is not written, a twiddle where none belongs or a value from another place shows in the bits."""
    hop, S = 5, 4
    m = n + (S - 1) * hop
    z = np.concatenate([R.constant_pairs(m, OFFSET), R.impulse_pairs(n, OFFSET)])
    d = Guarded(z.nbytes).upload(z)
    for kind in R.KINDS:
        obj = fsea.Spectra(n, hop, kind)
        jobs = [(0, m)] + ([(m, n)] if kind == R.Z else [])
        assert obj.segments(m) == S
        got = run_device(obj, d, z.size, *laid_out(obj, jobs))
        want = R.constant_spectrum(n, kind)
        assert same_float_bits(got[0], want), (n, kind, got[0][n // 2], want[n // 2], np.flatnonzero(got[0].view(np.uint32) != want.view(np.uint32))[:8])
        if kind == R.Z:
            assert same_float_bits(got[1], R.impulse_spectrum(n)), (n, np.flatnonzero(got[1] != 20.0)[:8])
        obj.close()
    d.check("the input is read, not written")
    d.free()


@pytest.mark.parametrize("n", SIZES)
def test_a_window_of_ones_gives_the_bits_of_none(cutouts, n):
    z, d_pairs = cutouts
    for kind in R.KINDS:
        plain, ones = fsea.Spectra(n, n // 2, kind), fsea.Spectra(n, n // 2, kind, np.ones(n, np.float32))
        jobs = [(1, 3 * n), (4, n)]
        a = run_device(plain, d_pairs, z.size, *laid_out(plain, jobs))
        b = run_device(ones, d_pairs, z.size, *laid_out(ones, jobs))
        assert all(same_float_bits(x, y) for x, y in zip(a, b)), kind
        plain.close()
        ones.close()


def test_a_nan_pair_reaches_its_own_job_alone():
    """One NaN pair: in the job's pair 0, in a pair two segments share, in its last covered pair, in the tail no segment
    covers, in front of the job and behind it.  The job's bins are NaN where spectra_ref.nan_bins says so -- all of them, or
    none -- and its neighbours in the table, one of which overlaps it in the input short of that pair, keep their bits."""
    n, hop = 256, 100
    m = n + 2 * hop + 7                                             # S = 3, seven pairs that no segment covers
    base = R.noise_cutout(m + 40, seed=9)
    g = Guarded(base.nbytes)
    obj = fsea.Spectra(n, hop, "z", fsea.window("hann", n))
    first = 11
    jobs = [(0, n), (first, m), (first + m, 20)]                    # a neighbour in front, one behind that has no segment
    table, n_power = laid_out(obj, jobs)
    clean = run_device(obj, g.upload(base), base.size, table, n_power)
    assert np.all(np.isfinite(clean[1]))
    places = {"pair 0": 0, "a shared pair": hop + 5, "the last covered pair": 2 * hop + n - 1, "the tail": m - 1, "in front": -1, "behind": m}
    for name, at in places.items():
        z = base.copy()
        z[first + at] = complex(np.nan, 1.0)
        got = run_device(obj, g.upload(z), z.size, table, n_power)
        named = R.nan_bins(m, n, hop, at) if 0 <= at < m else []
        want, _ = R.spectrum(z[first:first + m], n, hop, obj.kind, fsea.window("hann", n), OFFSET)
        assert np.flatnonzero(np.isnan(want)).tolist() == named, name
        assert np.flatnonzero(np.isnan(got[1])).tolist() == named, name
        if not named:
            assert same_float_bits(got[1], clean[1]), name
        if first + at >= n:                                         # the neighbour in front does not hold the pair
            assert same_float_bits(got[0], clean[0]), name
        assert got[2].size == 0
    g.check("the input is read, not written")
    g.free()
    obj.close()


def test_the_host_form_gives_the_bits_of_the_device_form(cutouts):
    z, d_pairs = cutouts
    L_ = fsea.hip_lib()
    for n, hop, kind in ((64, 32, "env"), (4096, 4000, "z"), (512, 300, "sq"), (2048, 2048, "fourth")):
        obj = fsea.Spectra(n, hop, kind, fsea.window("hann", n))
        jobs = [(1, 3 * n + 5), (0, n - 1), (z.size - 2 * n, 2 * n), (7, 0), (2, n)]
        table, n_power = laid_out(obj, jobs, gap=5)
        device = run_device(obj, d_pairs, z.size, table, n_power)
        power = np.full(n_power, np.frombuffer(bytes([FILL] * 4), np.float32)[0], np.float32)
        rc = L_.fsea_spectra_run_host(obj._p, z.ctypes.data, z.size, ctypes.addressof(table), len(table), OFFSET.real, OFFSET.imag,
                                      power.ctypes.data, n_power)
        assert rc == 0, L_.fsea_last_error_string()
        owned = np.zeros(n_power, bool)
        for j, dev in zip(table, device):
            assert same_float_bits(power[j.out_first:j.out_first + dev.size], dev)
            owned[j.out_first:j.out_first + dev.size] = True
        assert np.all(power[~owned].view(np.uint8) == FILL)         # only the jobs' ranges
        assert all(same_float_bits(h, dev) for h, dev in zip(obj.run(z, table, OFFSET), device))
        obj.close()


def test_two_streams_and_an_odd_pair_base(cutouts):
    """Calls with tables of different sizes alternate on two streams over one object: each its own result.  A buffer that
    begins at an odd pair of the allocation: 8-byte aligned is all d_pairs has to be."""
    z, d_pairs = cutouts
    n, hop = 256, 64
    obj = fsea.Spectra(n, hop, "sq")
    sync = fsea.Plan(128)                        # fsea_stream_synchronize wants a plan for its device
    s1, s2 = fsea.Stream(), fsea.Stream()
    jobs_a = [(1, 9000), (10, 300)]
    jobs_b = [(2, 255), (7, 5000), (0, 0), (4, 2049), (100, 256), (3, 700)]
    ref = {}
    for shift, jobs in ((0, jobs_a), (1, jobs_b)):                  # each table alone, on the default stream
        table, n_power = laid_out(obj, [(a + shift, m) for a, m in jobs], gap=0)
        ref[shift] = run_device(obj, d_pairs, z.size, table, n_power)
    runs = []
    for r in range(3):
        for jobs, stream, shift in ((jobs_a, s1, 0), (jobs_b, s2, 1)):
            table, n_power = laid_out(obj, jobs, gap=r)
            g = Guarded(4 * max(n_power, 1))
            obj.run_device(d_pairs.addr + 8 * shift, z.size - shift, table, g.addr, max(n_power, 1), offset=OFFSET, stream=stream)
            runs.append((shift, table, n_power, g))
    sync.synchronize(s1)
    sync.synchronize(s2)
    for shift, table, n_power, g in runs:
        back = g.payload(np.float32, (max(n_power, 1),))
        for j, want in zip(table, ref[shift]):
            assert same_float_bits(back[j.out_first:j.out_first + want.size], want), (shift, j.first_pair)
        g.check("two streams")
        g.free()
    for o in (s1, s2, sync, obj):
        o.close()


def test_refusals_name_the_job_and_write_nothing(cutouts):
    z, d_pairs = cutouts
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    n = 64
    obj = fsea.Spectra(n, 32, "z")
    n_power = 4096
    g = Guarded(4 * n_power)

    def refused(word, jobs, pairs=d_pairs.addr, m=z.size, off=(0.5, 0.5), out=g.addr, n_out=n_power):
        tab = (fsea.SpectraJob * len(jobs))(*[fsea.SpectraJob(*j) for j in jobs])
        rc = L_.fsea_spectra_run_device(obj._p, pairs, m, address(tab), len(jobs), off[0], off[1], out, n_out, None)
        assert rc == FSEA_EINVAL and word in err(), (word, rc, err())

    ok = [(0, 100, 0), (5, 200, 64)]
    refused(b"job 1: pairs", [(0, 100, 0), (z.size - 79, 80, 64)])                  # a span past the buffer
    refused(b"job 1: outputs", [(0, 100, 0), (5, 200, n_power - 63)])               # 64 powers from 63 in front of the end
    refused(b"the outputs of jobs 0 and 1 overlap", [(0, 100, 0), (5, 200, 63)])
    refused(b"the outputs of jobs 0 and 2 overlap", [(0, 400, 50), (5, 80, 200), (9, 64, 113)])
    refused(b"offset is not finite", ok, off=(np.nan, 0.5))
    refused(b"aligned", ok, pairs=d_pairs.addr + 4)
    refused(b"aligned", ok, out=g.addr + 2)
    refused(b"NULL buffer", ok, out=None)
    assert L_.fsea_spectra_run_device(obj._p, None, 0, None, 0, np.nan, 0.0, None, 0, None) == 0      # no jobs: a no-op
    assert np.all(g.payload(np.uint8, (4 * n_power,)) == FILL)
    g.check("refused calls")
    g.free()
    # and the same object still works, at the edge of what is accepted: a job that ends with the buffer, powers that end with n_power
    tab = (fsea.SpectraJob * 3)(fsea.SpectraJob(z.size - 100, 100, 0), fsea.SpectraJob(z.size, 0, 64), fsea.SpectraJob(0, 63, 1 << 40))
    got = run_device(obj, d_pairs, z.size, tab, 64)
    assert worst_over_bound(got[0], z[z.size - 100:], obj, None) <= 1.0 and got[1].size == 0 and got[2].size == 0
    obj.close()


# ---- end to end: a recording with one QPSK burst -------------------------------------------------------------------------------

N, ROWS, D, TAPS, RATE = X.N, 128, X.D, X.TAPS, 1536000
# First row, the row behind the last, the carrier's bin from the middle.  A quarter bin: the box's centre is a whole or a half
# bin, so the cut-out's carrier stands at least a quarter bin off its centre and the fourth-power line at least
# 4 * 0.25 * D / N * 256 = 4 bins of the spectrum off its middle, outside the guard of 2.
BURST = (20, 100, 150.25)
SYMBOL = 16 * D                   # samples a symbol: sixteen pairs of the cut-out, a main lobe of a few columns


def qpsk_recording():
    """int8 IQ: noise of sigma 1 and one QPSK burst of amplitude 60 on whole frames, half-sine symbols."""
    rng = np.random.default_rng(81)
    x = rng.normal(0.0, 1.0, N * ROWS) + 1j * rng.normal(0.0, 1.0, N * ROWS)
    t = np.arange(BURST[0] * N, BURST[1] * N)
    x[t] += R.psk(t.size, 4, SYMBOL, 0.0, 60.0, seed=5) * np.exp(2j * np.pi * (BURST[2] / N) * t)
    raw = np.empty(2 * N * ROWS)
    raw[0::2], raw[1::2] = x.real, x.imag
    return np.clip(np.rint(raw), -128, 127).astype(np.int8).view(np.uint8)


def test_tool_finds_the_fourth_power_line_of_a_qpsk_burst(tmp_path):
    qpsk_recording().tofile(tmp_path / "qpsk.raw")
    tool = os.path.join(BIN, "fsea-cutouts")
    common = [tool, str(tmp_path / "qpsk.raw"), "--size", str(N), "--flip", "--offset", str(X.DETECTOR[2]), "--min-rows", str(X.MIN_ROWS),
              "--gap-cols", "4", "--gap-rows", "2", "--window", "hann", "--decimation", str(D), "--taps", str(TAPS), "--rate", str(RATE), "--freq", "100",
              "--min-cols", "6"]      # the pedestal of the 8-bit samples is an event of its own, three columns at the centre: not this one
    plain = subprocess.run(common + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    out = tmp_path / "fourth"
    r = subprocess.run(common + ["--out", str(out), "--spectra", "256", "--spectra-kind", "fourth"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout, open(out / "spectra.txt").read(), open(out / "cutouts.txt").read())
    assert r.stdout == plain.stdout.rstrip("\n") + " spectra 1\n" and r.stdout.endswith(" spectra 1\n") and r.stderr == plain.stderr
    before, after = sorted(os.listdir(tmp_path / "plain")), sorted(os.listdir(out))
    assert after == sorted(before + ["spectra.txt"]) and len([f for f in before if f.endswith(".cf32")]) == 1
    for f in before:                                              # everything else is what it was, byte for byte
        assert open(tmp_path / "plain" / f, "rb").read() == open(out / f, "rb").read(), f
    event = [line.split() for line in open(out / "cutouts.txt").read().splitlines() if int(line.split()[9]) > 0]
    assert len(event) == 1
    number, col_first, col_last = int(event[0][0]), int(event[0][3]), int(event[0][4])
    lines = open(out / "spectra.txt").read().splitlines()
    assert len(lines) == 1
    fields = lines[0].split()
    assert int(fields[0]) == number and int(fields[1]) >= 8 and len(fields) == 6
    centre = (col_first + col_last) / 2 - N // 2                   # where the cut-out's centre stands, in bins of the recording
    offset_hz = (BURST[2] - centre) * RATE / N
    pair_rate = RATE / D
    line_hz, line_db = float(fields[4]), float(fields[5])
    print("offset", offset_hz, "line", line_hz, "dB", line_db)
    assert abs(line_hz - 4 * offset_hz) <= pair_rate / 256          # within one bin of four times the offset
    assert line_db > 10.0
    # and the file's spectrum is the restatement's of the pairs the tool wrote
    y = np.fromfile(out / ("cutout-%05d.cf32" % number), dtype=np.complex64)
    c = fsea.lowpass_taps(RATE, 0.4 * RATE / D, TAPS)
    pedestal = 0.5 * float(np.cumsum(c.astype(np.float32).astype(np.float64))[-1])
    want, _ = R.spectrum(y, 256, 128, R.FOURTH, fsea.window("hann", 256), complex(pedestal, pedestal))
    f = R.finish(want.astype(np.float32), 2, 0.99)
    assert int(fields[1]) == R.segments(y.size, 256, 128) and abs(f["peak_cycles"] * pair_rate - line_hz) <= 1e-3 * pair_rate / 256
    # once more at 512 bins, the plain kind: the radix-2 pass from the command line; the guard of z is 0
    out = tmp_path / "z512"
    r = subprocess.run(common + ["--out", str(out), "--spectra", "512", "--spectra-kind", "z"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout, open(out / "spectra.txt").read())
    assert r.stdout == plain.stdout.rstrip("\n") + " spectra 1\n" and r.stderr == plain.stderr
    assert sorted(os.listdir(out)) == after
    for f in before:
        assert open(tmp_path / "plain" / f, "rb").read() == open(out / f, "rb").read(), f
    lines = open(out / "spectra.txt").read().splitlines()
    assert len(lines) == 1
    fields = lines[0].split()
    assert int(fields[0]) == number and len(fields) == 6 and int(fields[1]) == R.segments(y.size, 512, 256) >= 1
    want, _ = R.spectrum(y, 512, 256, R.Z, fsea.window("hann", 512), complex(pedestal, pedestal))
    f = R.finish(want.astype(np.float32), 0, 0.99)
    assert abs(f["peak_cycles"] * pair_rate - float(fields[4])) <= 1e-3 * pair_rate / 512
