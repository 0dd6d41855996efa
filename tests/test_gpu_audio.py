"""GPU tier: cut-out audio (fsea_audio_*, kernel fsea_audio_tiles) and fsea-cutouts --audio.

Bit identity, no tolerance: a job's audio is tests/audio_ref.py's for the job's pairs -- the same terms with the same
roundings, the discriminator branch by branch, one chain per output over the taps ascending -- whatever first_pair is,
whatever other jobs share the call and in whatever order, for both kinds.  The shapes are the smallest at which the kernel
can still go wrong: decimations 1, 3, 8 and the largest, one tap, a usual filter and the longest, lengths round one output,
round one tile of T outputs (T is the object's own: 256 down to 56) and round two, one job of five tiles; odd and even
firsts; jobs that overlap in the input; one that ends with the buffer.  A single tap at D = 1 lays d itself open, so a
division or a square root that is not correctly rounded on the device shows there at once.  Inputs and outputs are guarded."""
import math
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea
from tests import audio_ref as A
from tests import demod_ref
from tests import extract_ref as X
from tests.conftest import ROOT
from tests.guarded import FILL, Guarded
from tests.jobs_common import address, pairs_of, pedestal, same_float_bits
from tests.jobs_common import run_device as run_placed
from tests.test_audio_host import (AUDIO_CUTOFF, CARRIER_BIN, D, D2, DEVIATION, L, L2, RATE, audio_taps, tone_check, tone_recording)

pytestmark = pytest.mark.gpu

OFFSET = 0.5 + 0.5j
GAIN = 0.75
BIN = os.path.join(ROOT, "frequensea_amd", "bin")
FSEA_EINVAL = -1
N_BUFFER = 5 * 4096 + 600
KINDS = (A.FM, A.AM)


def lengths(d, n_taps):
    t = A.tile(d, n_taps)
    return [0, 1, d - 1, d, t * d - 1, t * d, t * d + 1, 2 * t * d + d - 1, 5 * t * d - d // 2 - 1]


def sweep(d, n_taps):
    """(first_pair, n_pairs) per job: every length at an even and at an odd first, all of them overlapping in the buffer's
    first pairs; the longest job at an odd first ends with the buffer."""
    ns = lengths(d, n_taps)
    jobs = []
    for i, n in enumerate(ns):
        jobs.append((2 * (len(ns) - i), n))
        jobs.append((2 * i + 1, n))
    n = jobs[-1][1] - (N_BUFFER - jobs[-1][1] + 1) % 2           # a pair shorter where that makes its first odd
    jobs[-1] = (N_BUFFER - n, n)
    assert jobs[-1][0] % 2 == 1 and sum(jobs[-1]) == N_BUFFER and all(a + n <= N_BUFFER for a, n in jobs)
    return jobs


def taps_of(n_taps, seed=3):
    rng = np.random.default_rng(seed + n_taps)
    return rng.uniform(0.5, 1.5, n_taps) * rng.choice([-1.0, 1.0], n_taps) / n_taps


def laid_out(jobs, d, gap=3):
    """the jobs as a table with their outputs in table order, `gap` floats of fill between them; the floats in all"""
    at, rows = gap, []
    for a, n in jobs:
        rows.append(fsea.AudioJob(a, n, at))
        at += n // d + gap
    return (fsea.AudioJob * len(rows))(*rows), at


def run_device(obj, d_pairs, n_buffer, table, n_audio, offset=OFFSET, gain=GAIN, stream=0, wait=None):
    """one call into a guarded output pre-filled with FILL -> (one float32 array per job, the mask of floats no job owns)"""
    return run_placed(obj, d_pairs, n_buffer, table, n_audio, lambda j: j.n_pairs // obj.decimation, "audio", stream, wait,
                      offset=offset, gain=gain)


@pytest.fixture(scope="module")
def resident():
    z = pairs_of(31, N_BUFFER)
    d = Guarded(z.nbytes).upload(z)
    yield z, d
    d.check("the input is read, not written")
    d.free()


@pytest.mark.parametrize("n_taps", [1, 41, 512])
@pytest.mark.parametrize("d", [1, 3, 8, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_every_output_equals_the_restatement_bit_for_bit(resident, kind, d, n_taps):
    z, d_pairs = resident
    c = taps_of(n_taps)
    obj = fsea.Audio(kind, c, d)
    jobs = sweep(d, n_taps)
    table, n_audio = laid_out(jobs, d)
    got = run_device(obj, d_pairs, N_BUFFER, table, n_audio)
    differ = 0
    for k, (a, n) in enumerate(jobs):
        want = A.audio(z[a:a + n], kind, c, d, OFFSET, GAIN)
        assert want.size == n // d == got[k].size
        differ += int(np.count_nonzero(got[k].view(np.uint32) != want.view(np.uint32)))
    print("kind", kind, "D", d, "L", n_taps, "T", A.tile(d, n_taps), "outputs that differ:", differ)
    assert differ == 0
    if n_taps == 1 and d == 1:       # d itself: every output is (float)(gain c[0] d_i)
        dd = A.discriminator(z[jobs[-1][0]:], kind, OFFSET)
        assert same_float_bits(got[-1], (np.float64(GAIN) * (0.0 + c[0] * dd)).astype(np.float32))
    # the host form: the same bits, and only the jobs' own floats
    host = obj.run(z, table, OFFSET, GAIN)
    assert all(same_float_bits(h, g) for h, g in zip(host, got))
    obj.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_table_does_not_change_a_bit(resident, kind):
    """The same jobs permuted, each alone in a call, and scattered among 700 small jobs: identical bits per job."""
    z, d_pairs = resident
    d, n_taps = 3, 41
    c = taps_of(n_taps)
    obj = fsea.Audio(kind, c, d)
    jobs = sweep(d, n_taps)
    table, n_audio = laid_out(jobs, d)
    together = run_device(obj, d_pairs, N_BUFFER, table, n_audio)
    order = list(np.random.default_rng(6).permutation(len(jobs)))
    t2, n2 = laid_out([jobs[k] for k in order], d, gap=1)
    permuted = run_device(obj, d_pairs, N_BUFFER, t2, n2)
    for at, k in enumerate(order):
        assert same_float_bits(permuted[at], together[k]), k
    for k, j in enumerate(jobs):
        t1, n1 = laid_out([j], d, gap=0)
        assert same_float_bits(run_device(obj, d_pairs, N_BUFFER, t1, max(n1, 1))[0], together[k]), k
    small = [(11 * i + i % 2, 0 if i % 9 == 4 else 2 + (i * 131) % 900) for i in range(700)]
    big, where = list(small), {}
    for k, j in enumerate(jobs):
        big.insert(28 * k, j)
        where[k] = 28 * k
    assert all(big[at] == jobs[k] for k, at in where.items()) and len(big) == 700 + len(jobs)
    t3, n3 = laid_out(big, d, gap=2)
    among = run_device(obj, d_pairs, N_BUFFER, t3, n3)
    for k, at in where.items():
        assert same_float_bits(among[at], together[k]), k
    placed = set(where.values())
    for at, (a, n) in enumerate(big):
        if at not in placed and at % 7 == 0:                      # and the small ones are right too
            assert same_float_bits(among[at], A.audio(z[a:a + n], kind, c, d, OFFSET, GAIN)), (at, a, n)
    obj.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_pair_reaches_exactly_the_outputs_the_restatement_names(kind):
    """One NaN pair per buffer: at the job's pair 0, its last pair, the pairs behind a tile's first and last d, one pair in
    front of the job and one behind it.  The outputs audio_ref.nan_outputs names are NaN (the taps are all non-zero), every
    other output keeps the bits it has without the NaN; a NaN outside the job touches nothing."""
    d, n_taps = 3, 7
    t = A.tile(d, n_taps)
    assert t == 256
    c = taps_of(n_taps)
    obj = fsea.Audio(kind, c, d)
    n = 2 * t * d + 5 * d + 1
    base = pairs_of(32, n + 40)
    g = Guarded(base.nbytes)
    for first in (6, 9):
        table, n_audio = laid_out([(first, n)], d)
        clean = run_device(obj, g.upload(base), base.size, table, n_audio)[0]
        assert same_float_bits(clean, A.audio(base[first:first + n], kind, c, d, OFFSET, GAIN)) and np.all(np.isfinite(clean))
        # tile 1's span begins at d_ext[T D], i.e. pair T D - (L - 1); its last value is pair 2 T D - 1
        places = {"pair 0": 0, "the last pair": n - 1, "a tile's first d": t * d - (n_taps - 1), "a tile's last d": 2 * t * d - 1,
                  "the last d of tile 0": t * d - 1, "in front of the job": -1, "behind the job": n}
        for name, at in places.items():
            z = base.copy()
            z[first + at] = complex(np.nan, 1.0)
            got = run_device(obj, g.upload(z), z.size, table, n_audio)[0]
            want = A.audio(z[first:first + n], kind, c, d, OFFSET, GAIN)
            named = A.nan_outputs(n, kind, n_taps, d, at) if 0 <= at < n else []
            assert np.flatnonzero(np.isnan(want)).tolist() == named, (name, first)
            assert np.flatnonzero(np.isnan(got)).tolist() == named, (kind, name, first)
            keep = np.ones(got.size, bool)
            keep[named] = False
            assert same_float_bits(got[keep], clean[keep]), (kind, name, first)
            if not 0 <= at < n:
                assert named == [] and same_float_bits(got, clean), (kind, name, first)
    g.check("the input is read, not written")
    g.free()
    obj.close()


def test_refusals_name_the_job_and_write_nothing(resident):
    z, d_pairs = resident
    L_ = fsea.hip_lib()
    err = L_.fsea_last_error_string
    obj = fsea.Audio("fm", taps_of(41), 4)
    n_audio = 4096
    g = Guarded(4 * n_audio)

    def refused(word, jobs, pairs=d_pairs.addr, n=N_BUFFER, off=(0.5, 0.5), gain=1.0, out=g.addr, n_out=n_audio):
        tab = (fsea.AudioJob * len(jobs))(*[fsea.AudioJob(*j) for j in jobs])
        rc = L_.fsea_audio_run_device(obj._p, pairs, n, address(tab), len(jobs), off[0], off[1], gain, out, n_out, None)
        assert rc == FSEA_EINVAL and word in err(), (word, rc, err())

    ok = [(0, 40, 0), (5, 80, 10)]
    refused(b"job 1: pairs", [(0, 40, 0), (N_BUFFER - 79, 80, 10)])                  # a span past the buffer
    refused(b"job 1: outputs", [(0, 40, 0), (5, 80, n_audio - 19)])                  # 20 outputs from 19 in front of the end
    refused(b"the outputs of jobs 0 and 1 overlap", [(0, 40, 0), (5, 80, 9)])
    refused(b"the outputs of jobs 0 and 2 overlap", [(0, 400, 50), (5, 80, 10), (9, 4, 149)])
    refused(b"gain is not finite", ok, gain=np.inf)
    refused(b"gain is not finite", ok, gain=np.nan)
    refused(b"offset is not finite", ok, off=(np.nan, 0.5))
    refused(b"aligned", ok, pairs=d_pairs.addr + 4)
    refused(b"aligned", ok, out=g.addr + 2)
    refused(b"NULL buffer", ok, out=None)
    assert L_.fsea_audio_run_device(obj._p, None, 0, None, 0, np.nan, 0.0, np.nan, None, 0, None) == 0      # no jobs: a no-op
    assert np.all(g.payload(np.uint8, (4 * n_audio,)) == FILL)
    g.check("refused calls")
    g.free()
    # and the same object still works, at the edge of what is accepted: a job that ends with the buffer, outputs that end with n_audio
    tab = (fsea.AudioJob * 2)(fsea.AudioJob(N_BUFFER - 80, 80, 0), fsea.AudioJob(N_BUFFER, 0, 20))
    got = run_device(obj, d_pairs, N_BUFFER, tab, 20, gain=1.0)
    assert same_float_bits(got[0], A.audio(z[N_BUFFER - 80:], A.FM, taps_of(41), 4, OFFSET, 1.0)) and got[1].size == 0
    obj.close()


def test_two_streams_and_an_odd_pair_base(resident):
    """Calls with tables of different sizes alternate on two streams over one object: each its own result.  A buffer that
    begins at an odd pair of the allocation: 8-byte aligned is all d_pairs has to be."""
    z, d_pairs = resident
    c = taps_of(41)
    obj = fsea.Audio("am", c, 8)
    sync = fsea.Plan(128)                        # fsea_stream_synchronize wants a plan for its device
    s1, s2 = fsea.Stream(), fsea.Stream()
    jobs_a = [(1, 9000), (10, 300)]
    jobs_b = [(2, 70), (7, 5000), (0, 0), (4, 2049), (100, 8), (3, 7)]
    runs = []
    for r in range(3):
        for jobs, stream, shift in ((jobs_a, s1, 0), (jobs_b, s2, 1)):
            table, n_audio = laid_out(jobs, 8, gap=r)
            g = Guarded(4 * max(n_audio, 1))
            obj.run_device(d_pairs.addr + 8 * shift, N_BUFFER - shift, table, g.addr, max(n_audio, 1), offset=OFFSET, gain=GAIN, stream=stream)
            runs.append((jobs, shift, table, n_audio, g))
    sync.synchronize(s1)
    sync.synchronize(s2)
    for jobs, shift, table, n_audio, g in runs:
        back = g.payload(np.float32, (max(n_audio, 1),))
        for j, (a, n) in zip(table, jobs):
            assert same_float_bits(back[j.out_first:j.out_first + n // 8], A.audio(z[shift + a:shift + a + n], A.AM, c, 8, OFFSET, GAIN)), (a, n)
        g.check("two streams")
        g.free()
    for o in (s1, s2, sync, obj):
        o.close()


# ---- end to end: a recording with an FM burst that carries a tone and an AM burst

N, ROWS = X.N, 128
FM_BURST, AM_BURST = (10, 60, 200), (70, 120, -300)          # first row, the row behind the last, the carrier's bin from the middle
TONE = 1000.0


def bursts_recording():
    """int8 IQ at RATE: noise of sigma 1; an FM burst of amplitude 60 (DEVIATION Hz of a TONE Hz cosine) and an AM burst of
    carrier 50 at depth 0.5, each on whole frames at a whole bin.  The rows are Hann-windowed: neither burst is a line."""
    rng = np.random.default_rng(79)
    x = rng.normal(0.0, 1.0, N * ROWS) + 1j * rng.normal(0.0, 1.0, N * ROWS)
    for (f0, f1, k), make in ((FM_BURST, lambda n: A.fm_signal(n, RATE, TONE, DEVIATION, 60.0)),
                              (AM_BURST, lambda n: A.am_signal(n, RATE, TONE, 0.5, 50.0))):
        t = np.arange(f0 * N, f1 * N)
        x[t] += make(t.size) * np.exp(2j * np.pi * (k / N) * t)
    raw = np.empty(2 * N * ROWS)
    raw[0::2], raw[1::2] = x.real, x.imag
    return np.clip(np.rint(raw), -128, 127).astype(np.int8).view(np.uint8)


def test_end_to_end_a_tone_comes_out_of_its_burst():
    """plan -> cfar -> events -> extract_jobs -> extract -> audio on the device, both kinds over both cut-outs: the GPU audio
    is the restatement's for the pairs the extract left, bit for bit, and the FM burst's FM audio and the AM burst's AM audio
    pass the CPU tier's tone check."""
    raw = bursts_recording()
    plan = fsea.Plan(N, N, fsea.MODE_DB5_U8_DCFIX)
    plan.set_window(fsea.window("hann", N))
    rows = plan.exec_host(raw, ROWS, flip=True)
    plan.close()
    cfar, ev = fsea.Cfar(N), fsea.Events(N)
    cfar.set(*X.DETECTOR)
    runs = ev.runs(cfar.add(rows, mask=True), rows)
    events, _ = fsea.Events.link(runs, gap_cols=4, gap_rows=2, min_rows=X.MIN_ROWS)
    cfar.close()
    ev.close()
    ejobs, fits = fsea.extract_jobs(events, N, N, N * ROWS, L, D)
    print("events", [(int(e["row_first"]), int(e["row_last"]), int(e["col_first"]), int(e["col_last"])) for e in events], list(fits))
    assert events.size >= 2
    c = fsea.lowpass_taps(RATE, 0.4 * RATE / D, L)
    ex = fsea.Extract(c, D)
    laid, total = ex.layout(ejobs)
    d_iq, g_pairs = Guarded(raw.nbytes).upload(raw), Guarded(8 * total)
    ex.run_device(d_iq.addr, raw.size // 2, laid, g_pairs.addr, total, flip=True)
    spans = fsea.measure_jobs(laid, D, fsea.extract_lead(L, D) // D)
    off = pedestal(c) * (1 + 1j)
    c2 = audio_taps()
    pairs = None
    for kind, gain in ((A.FM, RATE / D / (2 * math.pi * DEVIATION)), (A.AM, 1.0)):
        obj = fsea.Audio(kind, c2, D2)
        table, n_audio = obj.layout([fsea.AudioJob(s.first_pair, s.n_pairs, 0) for s in spans])
        assert bytes(table) == bytes(fsea.audio_layout([fsea.AudioJob(s.first_pair, s.n_pairs, 9) for s in spans], D2)[0])
        got = run_device(obj, g_pairs, total, table, n_audio, offset=off, gain=gain)
        if pairs is None:
            pairs = g_pairs.payload(np.complex64, (total,))
        for k, j in enumerate(table):
            assert same_float_bits(got[k], A.audio(pairs[j.first_pair:j.first_pair + j.n_pairs], kind, c2, D2, off, gain)), (kind, k)
        # the burst of this kind: the event at its bin; the outputs whose taps lie inside the burst
        burst = FM_BURST if kind == A.FM else AM_BURST
        mine = [i for i, e in enumerate(events) if fits[i] and e["col_first"] <= N // 2 + burst[2] <= e["col_last"] and
                e["row_first"] <= burst[0] + 2 and e["row_last"] >= burst[1] - 3]
        assert len(mine) == 1, (kind, mine)
        k, e = mine[0], events[mine[0]]
        # the middle three fifths of the cut-out lie inside the burst whatever rows the box gained at its ends
        inside = got[k][got[k].size // 5:-(got[k].size // 5)]
        assert inside.size > 800
        centre = (int(e["col_first"]) + int(e["col_last"])) / 2 - N // 2           # where the job's centre stands, in bins
        tone_check(inside, kind, carrier_hz=(burst[2] - centre) * RATE / N)
        obj.close()
    g_pairs.check("the extract's output is read, not written")
    for o in (d_iq, g_pairs):
        o.free()
    ex.close()


def test_tool_writes_the_restatements_pcm(tmp_path):
    raw = bursts_recording()
    raw.tofile(tmp_path / "bursts.raw")
    tool = os.path.join(BIN, "fsea-cutouts")
    common = [tool, str(tmp_path / "bursts.raw"), "--size", str(N), "--flip", "--offset", str(X.DETECTOR[2]), "--min-rows", str(X.MIN_ROWS),
              "--gap-cols", "4", "--gap-rows", "2", "--window", "hann", "--decimation", str(D), "--taps", str(L), "--rate", str(RATE), "--freq", "100"]
    plain = subprocess.run(common + ["--out", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    c = fsea.lowpass_taps(RATE, 0.4 * RATE / D, L)
    off = pedestal(c) * (1 + 1j)
    for kind, name in ((A.FM, "fm"), (A.AM, "am")):
        out = tmp_path / name
        r = subprocess.run(common + ["--out", str(out), "--audio", name, "--audio-rate", str(RATE // D // D2), "--audio-taps", str(L2),
                                     "--audio-cutoff", str(AUDIO_CUTOFF), "--deviation", str(DEVIATION)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        before, after = sorted(os.listdir(tmp_path / "plain")), sorted(os.listdir(out))
        files = [f for f in before if f.endswith(".cf32")]
        wavs = [f[:-5] + ".wav" for f in files]
        assert len(files) >= 2 and after == sorted(before + wavs + ["audio.txt"])
        assert r.stdout == plain.stdout.rstrip("\n") + " audio %d\n" % len(files) and r.stderr == plain.stderr
        for f in before:                                          # everything else is what it was, byte for byte
            assert open(tmp_path / "plain" / f, "rb").read() == open(out / f, "rb").read(), f
        lines = open(out / "audio.txt").read().split("\n")
        assert lines[-1] == "" and len(lines) == len(files) + 1
        gain = RATE / D / (2 * math.pi * DEVIATION) if kind == A.FM else 1.0
        for line, f, w in zip(lines, files, wavs):
            y = np.fromfile(out / f, dtype=np.complex64)
            a = A.audio(y, kind, audio_taps(), D2, off, gain).astype(np.float64)
            if kind == A.AM:
                a = a - np.cumsum(a)[-1] / a.size                 # the sum in order, over the count
            data = open(out / w, "rb").read()
            assert data[:4] == b"RIFF" and data[8:16] == b"WAVEfmt " and data[36:40] == b"data" and len(data) == 44 + 2 * a.size
            assert int.from_bytes(data[4:8], "little") == 36 + 2 * a.size and int.from_bytes(data[40:44], "little") == 2 * a.size
            assert [int.from_bytes(data[i:j], "little") for i, j in ((16, 20), (20, 22), (22, 24), (24, 28), (28, 32), (32, 34), (34, 36))] == [
                16, 1, 1, RATE // D // D2, 2 * (RATE // D // D2), 2, 16]
            # nrf_player's conversion where its cast is defined; in front of the burst the discriminator sees noise and
            # swings past full scale, where the tool saturates
            inside = (a * 32000 < 32767) & (a * 32000 > -32768)
            samples = np.frombuffer(data[44:], dtype="<i2")
            assert inside.sum() > 0.9 * a.size and np.array_equal(samples[inside], demod_ref.pcm(a[inside])), w
            assert np.array_equal(samples[~inside], np.where(a[~inside] > 0, 32767, -32768)), w
            number = int(f[len("cutout-"):-len(".cf32")])
            assert line == "%d %.3f %d %.6f" % (number, RATE / D / D2, a.size, np.abs(a).max()), line
