"""GPU tier: the audio chain (fsea_demod_*, kernels fsea_demod_stage1_* / fsea_demod_fm / fsea_demod_deemph), the nrf
demodulators, decoder and player on top of it, against the reference's own outputs (tests/golden/demod_golden.npz) and
the numpy restatement (tests/demod_ref.py).

Tolerance: max |delta| <= 1e-8 on audio samples; the expected size is about 1e-10.  Error budget of one audio sample:
  - phase: the reference rotates by a running product whose error grows by about k eps (1e-11 after a 131072-sample
    block), the kernel by a phase seeded every 8 samples from the exactly reduced cycle count (a few eps); the rotated
    samples differ by ~1e-11.  WBFM's discriminator sees only the phase step, where the common error cancels; RAW sees
    it in full, scaled by the filter gain (~1): <= ~1e-11 per block (test_demod_host measures both restatements apart);
  - filters: the kernels sum the 51 / 41 products with fused multiply-adds in f64, the reference without; per output
    <= L eps sum|c| |x| ~ 51 * 1.1e-16 * 1.2 * 1 ~ 7e-15;
  - discriminator: the reference's expressions operation for operation (contraction off), so it differs only by its
    inputs' ~1e-14 relative error, amplified by 1 / |y1|^2 (|y1| >= ~0.05 on the captures) to <= ~1e-11;
  - de-emphasis: a chunked scan of v = v + alpha (x - v); each chunk's start value carries a few eps of the composed
    maps, and the recurrence contracts (|1 - alpha| = 0.71 at 48 kHz): ~1e-16.
A sample beyond 1e-8 would mean a discriminator branch flipped (real == imag / real > imag boundaries): at the
real == imag boundary the two branches give atan approximations 1.8e-4 apart, ~2e-6 in audio after the filters.
PCM: (int16_t)(audio * 32000) truncates, so an audio difference of 1e-10 flips a sample only within 3.2e-6 LSB of an
integer: the player's chunks equal the golden PCM to +-1 LSB, and the count of +-1 samples is reported (expected 0)."""
import ctypes
import math
import os
import threading
import time

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import demod_ref as R
from tests.test_demod_host import GOLDEN, MG, capture, expected_tone_amplitude, fm_tone_u8, tone_check

pytestmark = pytest.mark.gpu

MAX_ABS = 1e-8


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size:
        err = float(np.max(np.abs(got - want)))
        assert err <= MAX_ABS, (what, err)
        return err
    return 0.0


def dec_runs(rate):
    runs = [("%s_%d_%d" % ("wbfm" if t else "raw", rate, off), t, off, None) for t, off in MG.DEC_CONFIGS]
    return runs + [("chg_%d" % rate, 1, 50000, 100000)]


@pytest.mark.parametrize("rate", MG.RATES)
def test_nrf_decoder_matches_the_reference(gold, rate):
    L = nrf.nrf_lib()
    samples = np.ascontiguousarray(gold["block__raw"] ^ 0x80)
    worst = 0.0
    for tag, t, off, change in dec_runs(rate):
        dec = L.nrf_decoder_new(t, rate, 48000, off)
        ref = R.Decoder(t, rate, 48000, off, phase="exact")
        for k in range(MG.CALLS):
            if change is not None and k == 2:
                dec.contents.freq_shifter.contents.freq_offset = change
                ref.offset = change
            L.nrf_decoder_process(dec, samples.ctypes.data, samples.size // 2)
            m = dec.contents.audio_samples_length
            got = np.ctypeslib.as_array(dec.contents.audio_samples, shape=(m,)).copy()
            worst = max(worst, check(got, gold["dec__%s__out%d" % (tag, k)], (tag, k)))
            check(got, ref.process(samples), (tag, k, "numpy"))
            sh = dec.contents.freq_shifter.contents
            assert np.allclose([sh.cosine, sh.sine], gold["dec__%s__phase" % tag][k], rtol=0, atol=1e-9), (tag, k)
            # the audio buffer is the demodulator's, aliased
            dm = ctypes.cast(dec.contents.demodulator, ctypes.POINTER(nrf.NrfFmDemodulator if t else nrf.NrfRawDemodulator))
            assert ctypes.addressof(dm.contents.audio_samples.contents) == ctypes.addressof(dec.contents.audio_samples.contents)
            assert not dec.contents.samples_i and dec.contents.samples_length == 0
        L.nrf_decoder_free(dec)
    print("nrf_decoder at %d Hz: max |audio - reference| = %.2e" % (rate, worst))


def test_unknown_demodulate_type_leaves_audio_null(gold):
    L = nrf.nrf_lib()
    samples = np.ascontiguousarray(gold["block__raw"] ^ 0x80)
    dec = L.nrf_decoder_new(7, 5000000, 48000, 50000)
    L.nrf_decoder_process(dec, samples.ctypes.data, samples.size // 2)
    assert not dec.contents.audio_samples and dec.contents.audio_samples_length == 0
    sh = dec.contents.freq_shifter.contents
    assert np.allclose([sh.cosine, sh.sine], gold["dec__wbfm_5000000_50000__phase"][0], rtol=0, atol=1e-9)
    L.nrf_decoder_free(dec)


@pytest.mark.parametrize("rate", MG.RATES)
def test_nrf_demodulators_match_the_reference(gold, rate):
    L = nrf.nrf_lib()
    ins = MG.dm_inputs(gold["block__raw"], capture())
    for kind in ("raw", "wbfm"):
        new = L.nrf_raw_demodulator_new if kind == "raw" else L.nrf_fm_demodulator_new
        proc = L.nrf_raw_demodulator_process if kind == "raw" else L.nrf_fm_demodulator_process
        free = L.nrf_raw_demodulator_free if kind == "raw" else L.nrf_fm_demodulator_free
        dm = new(rate, 48000)
        if kind == "wbfm":
            assert dm.contents.ampl_conv == 48000 / (2 * math.pi * 75000)
            assert dm.contents.downsampler_i.contents.rate_mul == rate / 336000.0
        for k, (i, q) in enumerate(ins):
            i, q = np.ascontiguousarray(i), np.ascontiguousarray(q)
            proc(dm, i.ctypes.data, q.ctypes.data, i.size)
            m = dm.contents.audio_samples_length
            got = np.ctypeslib.as_array(dm.contents.audio_samples, shape=(m,)).copy()
            check(got, gold["dm__%s_%d__out%d" % (kind, rate, k)], (kind, rate, k))
        free(dm)


@pytest.mark.parametrize("kind", ["raw", "wbfm"])
def test_ragged_calls_continue_one_stream(kind):
    """Calls of 1, < 50, not a multiple of a tile, 131072 and more samples continue one signal (state carried), against the
    restatement with the same calls; reset() gives a fresh object's output bit for bit."""
    rate, off = 5000000, -120000
    lengths = [1, 7, 49, 3, 2049, 131072, 4097, 1, 131072 * 3 + 5]
    u = np.random.default_rng(1).integers(0, 256, 2 * sum(lengths), dtype=np.uint8)
    d = fsea.Demod(kind, rate)
    d.set_channel(0, off)
    ref = R.Decoder(1 if kind == "wbfm" else 0, rate, 48000, off, phase="exact")
    pos, first = 0, []
    for n in lengths:
        chunk = u[2 * pos:2 * (pos + n)]
        pos += n
        got = d.run_u8(chunk)[0]
        assert got.size == d.out_length(n)
        check(got, ref.process(chunk), (kind, n))
        first.append(got)
    d.reset()
    assert d.get_channel(0) == (off, 1.0, 0.0)
    fresh = fsea.Demod(kind, rate)
    fresh.set_channel(0, off)
    pos = 0
    for n in lengths[:6]:
        chunk = u[2 * pos:2 * (pos + n)]
        pos += n
        assert np.array_equal(d.run_u8(chunk), fresh.run_u8(chunk))
    d.close()
    fresh.close()


def test_one_call_near_the_cap():
    n = fsea.DEMOD_MAX_SAMPLES - 3
    u = np.random.default_rng(2).integers(0, 256, 2 * n, dtype=np.uint8)
    d = fsea.Demod("wbfm", 5000000)
    d.set_channel(0, 50000)
    got = d.run_u8(u)[0]
    check(got, R.Decoder(1, 5000000, 48000, 50000, phase="exact").process(u), "cap")
    with pytest.raises(fsea.FseaError):
        d.run_u8(np.zeros(2 * (fsea.DEMOD_MAX_SAMPLES + 1), dtype=np.uint8))
    d.close()


def test_offset_change_keeps_the_phase(gold):
    """set_channel with the phase get_channel returns: the new offset from the next call, the phase continuing."""
    samples = gold["block__raw"] ^ 0x80
    d = fsea.Demod("wbfm", 5000000)
    d.set_channel(0, 50000)
    outs = [d.run_u8(samples)[0] for _ in range(2)]
    off, c, s = d.get_channel(0)
    assert off == 50000 and abs(c * c + s * s - 1) < 1e-12
    assert np.allclose([c, s], gold["dec__chg_5000000__phase"][1], rtol=0, atol=1e-9)
    d.set_channel(0, 100000, c, s)
    outs.append(d.run_u8(samples)[0])
    for k in range(3):
        check(outs[k], gold["dec__chg_5000000__out%d" % k], k)
    d.close()


def test_rate_below_one():
    """rate_mul < 1 (the reference allows it): RAW 1 MHz -> 3 MHz, WBFM from 200 kHz."""
    u = np.random.default_rng(4).integers(0, 256, 2 * 20000, dtype=np.uint8)
    for kind, rin, rout in (("raw", 1000000, 3000000), ("wbfm", 200000, 48000), ("wbfm", 5000000, 3000000)):
        d = fsea.Demod(kind, rin, rout)
        d.set_channel(0, 10000)
        ref = R.Decoder(1 if kind == "wbfm" else 0, rin, rout, 10000, phase="exact")
        for n in (1, 7, 20000 - 8):
            chunk = u[:2 * n]
            check(d.run_u8(chunk)[0], ref.process(chunk), (kind, rin, rout, n))
        d.close()


@pytest.mark.parametrize("K", [1, 8, 64])
def test_channels_are_bit_identical_to_single_channel_runs(gold, K):
    samples = gold["block__raw"] ^ 0x80
    rng = np.random.default_rng(K)
    offsets = [int(o) for o in rng.integers(-2400000, 2400000, K)]
    phases = [(math.cos(a), math.sin(a)) for a in rng.uniform(0, 2 * math.pi, K)]
    multi = fsea.Demod("wbfm", 5000000, n_channels=K)
    for ch in range(K):
        multi.set_channel(ch, offsets[ch], *phases[ch])
    outs = [multi.run_u8(samples) for _ in range(2)]
    for ch in sorted(set([0, K - 1] + list(range(0, K, max(1, K // 8))))):
        one = fsea.Demod("wbfm", 5000000)
        one.set_channel(0, offsets[ch], *phases[ch])
        for k in range(2):
            assert np.array_equal(outs[k][ch], one.run_u8(samples)[0]), (K, ch, k)
        assert one.get_channel(0) == multi.get_channel(ch)
        one.close()
    ref = R.Decoder(1, 5000000, 48000, offsets[K - 1], phase="exact")
    ref.c, ref.s = phases[K - 1]
    for k in range(2):
        check(outs[k][K - 1], ref.process(samples), (K, k))
    multi.close()


def test_device_form_on_a_user_stream(gold):
    import torch
    raw = gold["block__raw"]
    d_iq = torch.from_numpy(raw.copy()).to("cuda")
    K = 8
    dev = fsea.Demod("wbfm", 5000000, n_channels=K)
    host = fsea.Demod("wbfm", 5000000, n_channels=K)
    for ch in range(K):
        dev.set_channel(ch, 25000 * ch - 100000)
        host.set_channel(ch, 25000 * ch - 100000)
    m = dev.out_length(raw.size // 2)
    s = torch.cuda.Stream()
    for _ in range(3):
        d_audio = torch.empty((K, m), dtype=torch.float64, device="cuda")
        dev.run_device(d_iq.data_ptr(), raw.size // 2, d_audio.data_ptr(), flip=True, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(d_audio.cpu().numpy(), host.run_u8(raw ^ 0x80))
    dev.close()
    host.close()


def test_threads_on_one_object_and_on_two(gold):
    samples = gold["block__raw"] ^ 0x80
    calls = 6
    # one object, two threads: calls are serialised; every call sees the same block, so the state after 2 * calls calls
    # is the same whatever the interleaving, and the next call equals a sequential object's bit for bit
    shared = fsea.Demod("wbfm", 5000000)
    shared.set_channel(0, 50000)
    errors = []

    def hammer():
        try:
            for _ in range(calls):
                shared.run_u8(samples)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    ts = [threading.Thread(target=hammer) for _ in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors
    seq = fsea.Demod("wbfm", 5000000)
    seq.set_channel(0, 50000)
    for _ in range(2 * calls):
        seq.run_u8(samples)
    assert np.array_equal(shared.run_u8(samples), seq.run_u8(samples))
    assert shared.get_channel(0) == seq.get_channel(0)
    # two objects, two threads, different signals: each equals its single-threaded run
    rng = np.random.default_rng(5)
    streams = [rng.integers(0, 256, 2 * 200000, dtype=np.uint8) for _ in range(2)]
    results = [None, None]

    def run(k):
        d = fsea.Demod("raw" if k else "wbfm", 5000000)
        d.set_channel(0, 30000 * (k + 1))
        results[k] = [d.run_u8(streams[k][2 * p:2 * (p + 50000)]) for p in range(0, 200000, 50000)]
        d.close()

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(2):
        d = fsea.Demod("raw" if k else "wbfm", 5000000)
        d.set_channel(0, 30000 * (k + 1))
        for j, p in enumerate(range(0, 200000, 50000)):
            assert np.array_equal(results[k][j], d.run_u8(streams[k][2 * p:2 * (p + 50000)])), (k, j)
        d.close()
    shared.close()
    seq.close()


def test_synthetic_fm_tone_on_the_gpu():
    rate, n = 5000000, 131072
    u = fm_tone_u8(rate, 3 * n)
    d = fsea.Demod("wbfm", rate)
    d.set_channel(0, 50000)
    audio = np.concatenate([d.run_u8(u[2 * n * k:2 * n * (k + 1)])[0] for k in range(3)])
    d.close()
    corr, amp = tone_check(audio)
    assert corr > 0.99, corr
    assert abs(amp / expected_tone_amplitude() - 1) < 0.03, (amp, expected_tone_amplitude())


# ---- the player ----------------------------------------------------------------------------------------------------


class NrfPlayerHead(ctypes.Structure):
    """The leading members of this build's nrf_player (include/nrf.h)."""
    _fields_ = [("demodulate_type", ctypes.c_int), ("device", ctypes.c_void_p),
                ("decoder", ctypes.POINTER(nrf.NrfDecoder)), ("gain", ctypes.c_float)]


def pop_chunks(L, player, count, timeout=10.0):
    """The next `count` chunks as (sequence, int16 array)."""
    buf = np.empty(8192, dtype=np.int16)
    seq = ctypes.c_long()
    out, t0 = [], time.time()
    while len(out) < count:
        n = L.nrf_player_pop_pcm(player, buf.ctypes.data, buf.size, ctypes.byref(seq))
        if n:
            out.append((seq.value, buf[:n].copy()))
        else:
            assert time.time() - t0 < timeout, "no PCM chunk within %.0f s" % timeout
            time.sleep(0.001)
    return out


@pytest.fixture
def replay(gold, tmp_path):
    L = nrf.nrf_lib()
    path = tmp_path / "rf-100.900-block.raw"
    gold["block__raw"].tofile(str(path))
    dev = L.nrf_device_new(100.9, str(path).encode())
    L.nrf_device_set_paused(dev, 1)
    yield L, dev
    L.nrf_device_free(dev)


def compare_pcm(got, want, what):
    assert got.shape == want.shape, what
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1, what
    print("%s: %d of %d samples differ by 1 LSB" % (what, int(np.count_nonzero(diff)), diff.size))
    assert np.count_nonzero(diff) <= 4, what


def test_player_chunks_match_the_reference_pcm(gold, replay, tmp_path, monkeypatch):
    L, dev = replay
    pcm_path = tmp_path / "out.raw"
    monkeypatch.setenv("NRF_PLAYER_PCM", str(pcm_path))
    player = L.nrf_player_new(dev, nrf.NRF_DEMODULATE_WBFM, 50000)
    chunks = pop_chunks(L, player, 2)
    assert [c[0] for c in chunks] == [0, 1]
    L.nrf_player_set_freq_offset(player, 100000)          # from the next block on: the golden change sequence
    chunks += pop_chunks(L, player, 1)
    assert chunks[2][0] == 2
    for k in range(3):
        compare_pcm(chunks[k][1], gold["dec__chg_5000000__pcm%d" % k], "chunk %d" % k)
    for k in range(2):
        compare_pcm(chunks[k][1], gold["dec__wbfm_5000000_50000__pcm%d" % k], "chunk %d" % k)
    head = ctypes.cast(player, ctypes.POINTER(NrfPlayerHead)).contents
    for g, want in ((0.5, 0.5), (2.0, 1.0), (-1.0, 0.0), (1.0, 1.0)):
        L.nrf_player_set_gain(player, g)
        assert head.gain == want
    L.nrf_player_free(player)
    written = np.fromfile(str(pcm_path), dtype="<i2")
    assert written.size >= 3 * 1258 and written.size % 1258 == 0
    assert np.array_equal(written[:3 * 1258], np.concatenate([c[1] for c in chunks]))


def test_player_queue_drops_the_oldest(replay):
    L, dev = replay
    player = L.nrf_player_new(dev, nrf.NRF_DEMODULATE_RAW, 50000)
    time.sleep(3.0)       # > NRF_PLAYER_QUEUE + 6 blocks at the 60 Hz replay, even at half that rate
    seqs = [s for s, _ in pop_chunks(L, player, nrf_queue())]
    assert seqs[0] > 0 and seqs == list(range(seqs[0], seqs[0] + nrf_queue()))
    L.nrf_player_free(player)


def nrf_queue():
    return 64          # NRF_PLAYER_QUEUE (include/nrf.h)


def test_player_create_free_cycles_while_replaying(replay):
    L, dev = replay
    for k in range(20):
        player = L.nrf_player_new(dev, nrf.NRF_DEMODULATE_WBFM, 50000 + 1000 * k)
        time.sleep(0.005 * (k % 5))
        L.nrf_player_free(player)
    player = L.nrf_player_new(dev, nrf.NRF_DEMODULATE_WBFM, 50000)
    assert [s for s, _ in pop_chunks(L, player, 2)] == [0, 1]
    L.nrf_player_free(player)
