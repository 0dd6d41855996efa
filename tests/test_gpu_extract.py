"""GPU tier: event cut-outs (fsea_extract_*, kernel fsea_extract_u8 in its three LDS sizes) and fsea-cutouts.

Bit identity, no tolerance: a job's pairs are what a freshly reset fsea.Zoom(c, D, 128) gives for the job's slice of the
recording with the job's own cycles_per_sample, phase0_cycles and sample_offset (pairs=True) -- the same staging arithmetic,
the same phase-major image, one FMA chain per output -- whatever other jobs share the call, whatever their order and
whatever `first` mod 8 is.  The shapes are the smallest at which the kernel can still go wrong: lengths round one and two
tiles of ZOOM_TILE_OUTPUTS, jobs shorter than D and than the filter, every alignment of `first`, a job that ends with the
recording, a table long enough for the bisection to take every turn."""
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import extract_ref as R
from tests.conftest import ROOT
from tests.guarded import FILL, Guarded
from tests.test_gpu_zoom import lowpass_like_taps

pytestmark = pytest.mark.gpu

T = fsea.ZOOM_TILE_OUTPUTS
CASES = [(1, 21), (2, 1), (3, 41), (16, 97), (25, 97), (64, 512)]       # 18 KiB of LDS: the first four; 36 KiB; 69 KiB
CPS = (0.0, -0.12, 0.37, 1.75)
BIN = os.path.join(ROOT, "frequensea_amd", "bin")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def zoom_pairs(zoom, iq, j, flip):
    """the yardstick: the zoom, reset, on the job's slice"""
    zoom.reset()
    part = iq[2 * j.first:2 * (j.first + j.n_samples)]
    return zoom.run(part, j.cycles_per_sample, j.phase0_cycles, j.sample_offset, flip=bool(flip), pairs=True)[1]


def sweep_jobs(D, L):
    """(jobs, n_iq): the lengths of the sweep at firsts 0, 8, 3, 13 in turn, overlapping in the input, each with its own
    centre, phase and stream position; one job at stream position 2^52 - n; the last one ends with the recording at a first
    that is no multiple of 8."""
    lengths = [0, D - 1, D, (T - 1) * D, T * D, T * D + 1, (2 * T + 1) * D + D - 1, max(L - 2, 0)]
    n_iq = max(lengths) + 13 + 5
    last = T * D + 1
    while (n_iq - last) % 8 == 0:
        n_iq += 1
    jobs = []
    for i, n in enumerate(lengths):
        jobs.append(fsea.ExtractJob((0, 8, 3, 13)[i % 4], n, 1234563 + 1000 * i, CPS[i % 4], 0.3 * (i % 3), 0))
    n = (T + 1) * D + 2
    jobs.append(fsea.ExtractJob(5, n, (1 << 52) - n, -0.12, 0.0, 0))
    jobs.append(fsea.ExtractJob(n_iq - last, last, 77, 0.37, 0.25, 0))
    assert all(j.sample_offset != j.first and j.sample_offset % 8 for j in jobs[:-2]) and (n_iq - last) % 8
    return jobs, n_iq


def laid_out(ex, jobs, order):
    """the jobs with out_first from a layout in `order`: the table's order is not the outputs' -> (table, total pairs)"""
    permuted, total = ex.layout([fsea.ExtractJob.from_buffer_copy(jobs[k]) for k in order])
    table = [fsea.ExtractJob.from_buffer_copy(j) for j in jobs]
    for k, p in zip(order, permuted):
        table[k].out_first = p.out_first
    return table, total


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("D,L", CASES)
def test_every_job_equals_the_zoom_bit_for_bit(D, L, flip):
    c = lowpass_like_taps(L, 100 * D + L)
    ex, zoom = fsea.Extract(c, D), fsea.Zoom(c, D, 128)
    jobs, n_iq = sweep_jobs(D, L)
    iq = np.random.default_rng(1000 * D + L + flip).integers(0, 256, 2 * n_iq, dtype=np.uint8)
    order = [5, 0, 9, 2, 7, 1, 8, 3, 6, 4]
    table, total = laid_out(ex, jobs, order)
    assert [j.out_first for j in table] != sorted(j.out_first for j in table)
    d_iq, g_pairs = Guarded(iq.nbytes).upload(iq), Guarded(8 * total)
    ex.run_device(d_iq.addr, n_iq, table, g_pairs.addr, total, flip=bool(flip))
    got = g_pairs.payload(np.complex64, (total,))
    g_pairs.check("sweep D=%d L=%d" % (D, L))
    d_iq.check("the input is read, not written")
    for i, j in enumerate(table):
        want = zoom_pairs(zoom, iq, j, flip)
        assert want.size == j.n_samples // D == ex.out_pairs(j.n_samples)
        assert np.array_equal(bits(got[j.out_first:j.out_first + want.size]), bits(want)), (D, L, flip, i, j.n_samples, j.first)
    # the host form lays the same jobs out in table order and gives the same pairs
    for i, (j, mine) in enumerate(zip(table, ex.run(iq, jobs, flip=bool(flip)))):
        assert np.array_equal(bits(mine), bits(got[j.out_first:j.out_first + mine.size])), (D, L, flip, i, "host form")
    for o in (d_iq, g_pairs):
        o.free()
    ex.close()
    zoom.close()


def test_grouping_and_order_do_not_change_a_bit():
    D, L = 16, 97
    c = lowpass_like_taps(L, 7)
    ex = fsea.Extract(c, D)
    jobs, n_iq = sweep_jobs(D, L)
    iq = np.random.default_rng(5).integers(0, 256, 2 * n_iq, dtype=np.uint8)
    together = ex.run(iq, jobs, flip=True)
    order = list(np.random.default_rng(6).permutation(len(jobs)))
    permuted = ex.run(iq, [jobs[k] for k in order], flip=True)
    for k, mine in zip(order, permuted):
        assert np.array_equal(bits(mine), bits(together[k])), k
    for k, j in enumerate(jobs):
        alone = ex.run(iq, [j], flip=True)[0]
        assert np.array_equal(bits(alone), bits(together[k])), k
    ex.close()


def test_many_small_jobs_find_their_records():
    """1024 jobs of 3 D + 1 samples, every seventh one empty: 878 records, one tile each, so every workgroup's bisection
    ends at another record."""
    D, L, n_jobs = 16, 97, 1024
    c = lowpass_like_taps(L, 11)
    ex, zoom = fsea.Extract(c, D), fsea.Zoom(c, D, 128)
    n = 3 * D + 1
    n_iq = 5 * n_jobs + n + 3
    iq = np.random.default_rng(12).integers(0, 256, 2 * n_iq, dtype=np.uint8)
    jobs = [fsea.ExtractJob(5 * i, 0 if i % 7 == 3 else n, 99 + 3 * i, ((i * 37) % 201 - 100) / 256.0, 0.0, 0) for i in range(n_jobs)]
    got = ex.run(iq, jobs)
    for i, (j, mine) in enumerate(zip(jobs, got)):
        want = zoom_pairs(zoom, iq, j, 0)
        assert mine.size == want.size == (0 if i % 7 == 3 else 3)
        assert np.array_equal(bits(mine), bits(want)), i
    ex.close()
    zoom.close()


def test_nothing_outside_the_jobs_is_written_and_nothing_outside_the_input_read():
    D, L = 3, 41
    c = lowpass_like_taps(L, 13)
    ex = fsea.Extract(c, D)
    jobs, n_iq = sweep_jobs(D, L)
    iq = np.random.default_rng(14).integers(0, 256, 2 * n_iq, dtype=np.uint8)
    table, total = ex.layout(jobs)
    owned = np.zeros(total, bool)
    for j in table:
        owned[j.out_first:j.out_first + j.n_samples // D] = True
    assert 0 < (~owned).sum()                                   # odd outputs leave padding pairs
    results = []
    for fill in (FILL, 0x00):
        d_iq, g_pairs = Guarded(iq.nbytes, fill=fill).upload(iq), Guarded(8 * total)
        ex.run_device(d_iq.addr, n_iq, table, g_pairs.addr, total, flip=True)
        back = g_pairs.payload(np.uint8, (total, 8))
        g_pairs.check("a payload of exactly total_pairs pairs")
        d_iq.check("input")
        assert np.all(back[~owned] == FILL)                     # the padding between the jobs still holds the fill
        results.append(back[owned].copy())
        d_iq.free()
        g_pairs.free()
    assert np.array_equal(results[0], results[1])               # what lies round the input does not reach the output
    ex.close()


def test_forms_streams_and_lifetimes():
    D, L = 25, 97
    c = lowpass_like_taps(L, 15)
    ex = fsea.Extract(c, D)
    jobs, n_iq = sweep_jobs(D, L)
    iq = np.random.default_rng(16).integers(0, 256, 2 * n_iq, dtype=np.uint8)
    host = ex.run(iq, jobs, flip=True)
    # two calls with different tables, queued back to back on two streams: each its own result
    table_a, total_a = ex.layout(jobs)
    other = [fsea.ExtractJob.from_buffer_copy(j) for j in reversed(jobs[:6])]
    for j in other:
        j.cycles_per_sample += 0.05
    table_b, total_b = ex.layout(other)
    want_b = ex.run(iq, other, flip=True)
    sync = fsea.Plan(128)                        # fsea_stream_synchronize wants a plan for its device
    s1, s2 = fsea.Stream(), fsea.Stream()
    d_iq = fsea.DeviceBuffer(iq.nbytes).upload(iq)
    g_a, g_b = Guarded(8 * total_a), Guarded(8 * total_b)
    ex.run_device(d_iq.ptr.value, n_iq, table_a, g_a.addr, total_a, flip=True, stream=s1)
    ex.run_device(d_iq.ptr.value, n_iq, table_b, g_b.addr, total_b, flip=True, stream=s2)
    sync.synchronize(s1)
    sync.synchronize(s2)
    got_a, got_b = g_a.payload(np.complex64, (total_a,)), g_b.payload(np.complex64, (total_b,))
    for j, want in zip(table_a, host):
        assert np.array_equal(bits(got_a[j.out_first:j.out_first + want.size]), bits(want))
    for j, want in zip(table_b, want_b):
        assert np.array_equal(bits(got_b[j.out_first:j.out_first + want.size]), bits(want))
    assert not np.array_equal(bits(want_b[0]), bits(host[5]))
    for g in (g_a, g_b):
        g.check("two streams")
        g.free()
    # a call whose jobs have no output is a no-op; one with none at all too
    assert [a.size for a in ex.run(iq, [fsea.ExtractJob(3, D - 1, 0, 0.1, 0.0, 0)])] == [0] and ex.run(iq, []) == []
    d_iq.free()
    for o in (s1, s2, sync, ex):
        o.close()
    for k in range(4):
        e = fsea.Extract(c[:L - k], D - k)
        assert (e.n_taps, e.decimation) == (L - k, D - k)
        assert e.run(iq, jobs[4:5])[0].size == jobs[4].n_samples // (D - k)
        e.close()


@pytest.fixture(scope="module")
def detected():
    """plan (dB rows) -> Cfar -> Events.runs -> link -> extract_jobs -> Extract.run on the three bursts, once"""
    raw = R.recording()
    plan = fsea.Plan(R.N, R.N, fsea.MODE_DB5_U8_DCFIX)
    rows = plan.exec_host(raw, R.ROWS, flip=True)
    plan.close()
    cfar, ev = fsea.Cfar(R.N), fsea.Events(R.N)
    cfar.set(*R.DETECTOR)
    mask = cfar.add(rows, mask=True)
    runs = ev.runs(mask, rows)
    events, _ = fsea.Events.link(runs, min_rows=R.MIN_ROWS)
    cfar.close()
    ev.close()
    jobs, fits = fsea.extract_jobs(events, R.N, R.N, R.N * R.ROWS, R.TAPS, R.D)
    c = fsea.lowpass_taps(1.0, 0.4 / R.D, R.TAPS)
    ex = fsea.Extract(c, R.D)
    cutouts = ex.run(raw, [j for j, f in zip(jobs, fits) if f], flip=True)
    ex.close()
    return raw, runs, events, jobs, fits, cutouts, c


def test_end_to_end_every_burst_comes_out_at_the_centre_of_its_cutout(detected):
    raw, runs, events, jobs, fits, cutouts, c = detected
    assert events.size == 3 and list(fits) == [1, 1, 1]                     # one fitting job per burst
    want, want_fits = R.jobs(events, R.N, R.N, R.N * R.ROWS, R.TAPS, R.D)
    got = np.frombuffer(jobs, dtype=R.JOB)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.array_equal(fits, want_fits)
    run_in = R.lead(R.TAPS, R.D) // R.D
    for e, j, y, burst in zip(events, jobs, cutouts, R.BURSTS):
        assert e["col_first"] <= R.N // 2 + burst[2] <= e["col_last"] and e["row_first"] < burst[1] and e["row_last"] >= burst[0]
        assert y.size == j.n_samples // R.D > run_in
        k = R.peak_bin_inside_the_burst(y[run_in:], j.first, burst)
        assert abs(k) <= 1, (burst, k)
        # the same with the 0.5 + 0.5j the shifter's samples rest on taken off: only then the largest bin is the emission.  It
        # stands where the tone's column lies from the middle of the detected box (0 for a box centred on it), +-1
        k = R.peak_bin_inside_the_burst(y[run_in:], j.first, burst, rest=(0.5 + 0.5j) * c.sum())
        want = R.residual_bin(e, burst, R.inside_count(j.first, y.size, burst))
        print("burst", burst, "box", e["col_first"], e["col_last"], "peak bin", k, "expected", want)
        assert abs(k - want) <= 1, (burst, k, want, "without the shifter's 0.5 + 0.5j")


def test_tool_writes_the_python_paths_cutouts(detected, tmp_path):
    raw, runs, events, jobs, fits, cutouts, c = detected
    raw.tofile(tmp_path / "bursts.raw")
    out = tmp_path / "cut"
    rate, freq = 8000000.0, 100.0
    r = subprocess.run([os.path.join(BIN, "fsea-cutouts"), str(tmp_path / "bursts.raw"), "--size", str(R.N), "--flip", "--offset",
                        str(R.DETECTOR[2]), "--min-rows", str(R.MIN_ROWS), "--decimation", str(R.D), "--rate", "8000000", "--freq", "100",
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fitting = int(fits.sum())
    assert r.stdout == "rows %d runs %d events %d cutouts %d skipped %d\n" % (R.ROWS, runs.size, events.size, fitting, events.size - fitting)
    files = sorted(f for f in os.listdir(out) if f.endswith(".cf32"))
    assert files == ["cutout-%05d.cf32" % i for i in range(events.size) if fits[i]] and len(files) == 3
    run_in = R.lead(R.TAPS, R.D) // R.D
    for name, y in zip(files, cutouts):
        assert open(out / name, "rb").read() == y[run_in:].tobytes(), name
    lines = open(out / "cutouts.txt").read().split("\n")
    assert lines[-1] == "" and len(lines) == events.size + 1
    for i, (line, e, j, y) in enumerate(zip(lines, events, jobs, cutouts)):
        mhz = freq + ((int(e["col_first"]) + int(e["col_last"])) / 2 - R.N // 2) * rate / R.N / 1e6
        assert line == "%d %d %d %d %d %d %d %.6f %.3f %d %d 0" % (i, e["row_first"], e["row_last"], e["col_first"], e["col_last"], j.first,
                                                                 j.n_samples, mhz, rate / R.D, y.size - run_in, fits[i]), line
    # cut short: the same events, every cut-out 4096 samples at most and marked so
    r = subprocess.run([os.path.join(BIN, "fsea-cutouts"), str(tmp_path / "bursts.raw"), "--size", str(R.N), "--flip", "--offset",
                        str(R.DETECTOR[2]), "--min-rows", str(R.MIN_ROWS), "--decimation", str(R.D), "--max-samples", "4096",
                        "--max-events", "2", "--out", str(out) + "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "rows %d runs %d events 3 cutouts 2 skipped 1\n" % (R.ROWS, runs.size)
    for i in range(2):
        data = open(str(out) + "2/cutout-%05d.cf32" % i, "rb").read()
        assert data == cutouts[i][run_in:4096 // R.D].tobytes()
    lines = open(str(out) + "2/cutouts.txt").read().split("\n")
    assert [line.split()[-3:] for line in lines[:3]] == [[str(4096 // R.D - run_in), "1", "1"]] * 2 + [["0", "0", "0"]]
