"""The audio chain without a GPU: the numpy restatement (tests/demod_ref.py) and the host downsampler of libfsea_nrf.so
against the reference's recorded outputs (tests/golden/demod_golden.npz, written by make_demod_golden.py from the
reference's own nrf.c), the index tables, a synthetic FM known-answer case, argument errors of fsea_demod_* and the
layout of the four reference structs."""
import ctypes
import hashlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import demod_ref as R
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "demod_golden.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_demod_golden as MG  # noqa: E402  (the recorded configurations and inputs)

FSEA_EINVAL = -1
FSEA_ENODEVICE = -2
TAU_ = 2 * math.pi


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def capture():
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_golden.npz")) as z:
        return z["rf_100p900_1__raw"]


def test_header_caps_match_the_binding():
    text = open(os.path.join(ROOT, "include", "fsea.h")).read()
    assert int(re.search(r"#define FSEA_DEMOD_MAX_CHANNELS (\d+)", text).group(1)) == fsea.DEMOD_MAX_CHANNELS
    assert "#define FSEA_DEMOD_MAX_SAMPLES (1 << 24)" in text and fsea.DEMOD_MAX_SAMPLES == 1 << 24
    assert re.search(r"FSEA_DEMOD_RAW = 0, FSEA_DEMOD_WBFM = 1", text)


def test_numpy_downsampler_matches_the_reference(gold):
    x = MG.ds_input(gold["block__raw"])
    for rin, rout, cutoff, length in MG.DS_CONFIGS:
        tag = "ds__%d_%d" % (rin, rout)
        d = R.Downsampler(rin, rout, cutoff, length)
        pos = 0
        for k, n in enumerate(MG.DS_LENGTHS):
            y = d.process(x[pos:pos + n])
            pos += n
            assert y.size == int(gold[tag + "__len%d" % k]), (tag, k)
            got = y[gold[tag + "__idx%d" % k]]
            want = gold[tag + "__out%d" % k]
            assert np.max(np.abs(got - want), initial=0.0) <= 1e-12, (tag, k)


def test_host_downsampler_is_the_references_bit_for_bit(gold):
    L = nrf.nrf_lib()
    x = MG.ds_input(gold["block__raw"])
    for rin, rout, cutoff, length in MG.DS_CONFIGS:
        tag = "ds__%d_%d" % (rin, rout)
        d = L.nrf_downsampler_new(rin, rout, cutoff, length)
        assert d.contents.rate_mul == rin / float(rout)
        pos = 0
        for k, n in enumerate(MG.DS_LENGTHS):
            chunk = np.ascontiguousarray(x[pos:pos + n])
            pos += n
            L.nrf_downsampler_process(d, chunk.ctypes.data, n)
            m = d.contents.out_length
            assert m == int(gold[tag + "__len%d" % k])
            y = np.ctypeslib.as_array(d.contents.out_samples, shape=(m,)).copy() if m else np.zeros(0)
            assert np.array_equal(y[gold[tag + "__idx%d" % k]], gold[tag + "__out%d" % k]), (tag, k)
            assert np.array_equal(MG.sha(y), gold[tag + "__sha%d" % k]), (tag, k)
        L.nrf_downsampler_free(d)


def test_index_tables_are_the_accumulated_floor():
    """The tables the GPU uses (built by the same accumulation in fsea_demod.hip) against the reference's loop, for every
    recorded rate and call length, plus the decoder's chains at both rates."""
    rates = [rin / float(rout) for rin, rout, _, _ in MG.DS_CONFIGS] + [5e6 / 336000, 1e7 / 336000, 336000 / 48000.0]
    for r in rates:
        for n in MG.DS_LENGTHS + [131072, 8808, 4404, 262144 + 3]:
            want = []
            t = 0.0
            for _ in range(int(math.floor(n / r))):
                want.append(int(math.floor(t)))
                t += r
            assert np.array_equal(R.index_table(n, r), np.array(want, dtype=np.int64)), (r, n)
    # the accumulation and j * rate_mul part ways: floor(t) differs from floor(j * r) somewhere
    r = 1e7 / 336000
    idx = R.index_table(1 << 20, r)
    assert np.any(idx != np.floor(np.arange(idx.size) * r).astype(np.int64))


def test_numpy_demodulators_match_the_reference(gold):
    ins = MG.dm_inputs(gold["block__raw"], capture())
    for rate in MG.RATES:
        for kind in ("raw", "wbfm"):
            dm = R.RawDemodulator(rate, 48000) if kind == "raw" else R.FmDemodulator(rate, 48000)
            for k, (i, q) in enumerate(ins):
                got = dm.process(i, q)
                want = gold["dm__%s_%d__out%d" % (kind, rate, k)]
                assert got.shape == want.shape
                assert np.max(np.abs(got - want), initial=0.0) <= 1e-12, (kind, rate, k)


def test_numpy_decoder_matches_the_reference(gold):
    samples = gold["block__raw"] ^ 0x80
    assert gold["dec__wbfm_5000000_50000__out0"].size == 1258 and gold["dec__raw_5000000_50000__out0"].size == 1258
    assert gold["dec__wbfm_10000000_50000__out0"].size == 629
    for rate in MG.RATES:
        runs = [("%s_%d_%d" % ("wbfm" if t else "raw", rate, off), t, off, None) for t, off in MG.DEC_CONFIGS]
        runs.append(("chg_%d" % rate, 1, 50000, 100000))
        for tag, t, off, change in runs:
            dec = R.Decoder(t, rate, 48000, off)
            for k in range(MG.CALLS):
                if change is not None and k == 2:
                    dec.offset = change
                got = dec.process(samples)
                want = gold["dec__%s__out%d" % (tag, k)]
                assert np.max(np.abs(got - want)) <= 1e-12, (tag, k)
                assert np.array_equal(R.pcm(want), gold["dec__%s__pcm%d" % (tag, k)])
                assert np.allclose([dec.c, dec.s], gold["dec__%s__phase" % tag][k], rtol=0, atol=1e-12)


def test_exact_phase_differs_from_the_running_product_by_rounding_only(gold):
    """The project's phase (exactly reduced cycle count) against the reference's running product: about 1e-11 in the
    rotated samples after a block, and below 1e-10 in the decoded audio."""
    u8 = gold["block__raw"] ^ 0x80
    i, q = R.convert(u8[0::2]), R.convert(u8[1::2])
    ri, rq, rc, rs = R.rotate_reference(i, q, 50000, 5000000, 1.0, 0.0)
    ei, eq, ec, es = R.rotate_exact(i, q, 50000, 5000000, 1.0, 0.0)
    assert 0 < np.max(np.abs(ri - ei) + np.abs(rq - eq)) < 1e-10
    assert abs(rc - ec) + abs(rs - es) < 1e-10
    for t in (0, 1):
        a, b = R.Decoder(t, 5000000, 48000, 50000), R.Decoder(t, 5000000, 48000, 50000, phase="exact")
        for _ in range(3):
            assert np.max(np.abs(a.process(u8) - b.process(u8))) < 1e-10


def fm_tone_u8(in_rate, n, offset=50000, tone=1000.0, dev=75000.0, seed=0):
    """A 1 kHz tone, FM-modulated at 75 kHz deviation, `offset` Hz off centre, quantised to offset-binary u8 the way the
    decoder reads it (b / 128 - 0.995)."""
    k = np.arange(n)
    phase = TAU_ * (-offset) * k / in_rate + (dev / tone) * np.sin(TAU_ * tone * k / in_rate)
    amp = 0.7
    rng = np.random.default_rng(seed)
    i = amp * np.cos(phase) + rng.normal(0, 0.004, n)
    q = amp * np.sin(phase) + rng.normal(0, 0.004, n)
    u = np.empty(2 * n, dtype=np.uint8)
    u[0::2] = np.clip(np.rint((i + 0.995) * 128.0), 0, 255).astype(np.uint8)
    u[1::2] = np.clip(np.rint((q + 0.995) * 128.0), 0, 255).astype(np.uint8)
    return u


def tone_check(audio, out_rate=48000, tone=1000.0, dev=75000.0, settle=200):
    """(correlation with the best-fitting 1 kHz sinusoid, that sinusoid's amplitude) after `settle` samples."""
    a = audio[settle:]
    t = np.arange(a.size) / out_rate
    basis = np.stack([np.sin(TAU_ * tone * t), np.cos(TAU_ * tone * t), np.ones_like(t)], axis=1)
    coef, *_ = np.linalg.lstsq(basis, a, rcond=None)
    fit = basis @ coef
    corr = np.corrcoef(a - coef[2], fit - coef[2])[0, 1]
    return corr, math.hypot(coef[0], coef[1])


def expected_tone_amplitude(out_rate=48000, tone=1000.0, dev=75000.0):
    """The discriminator's output for a frequency deviation f at 336000 samples/s is about 2 pi f / 336000 * ampl_conv
    (atan of the phase step), ampl_conv = out / (2 pi 75000); the audio low-pass passes 1 kHz at ~1, and de-emphasis
    v += alpha (x - v) has gain |alpha / (1 - (1 - alpha) e^{-i w})| at w = 2 pi 1000 / out."""
    ampl_conv = out_rate / (TAU_ * 75000)
    alpha = 1.0 / (1.0 + out_rate * 50.0 / 1e6)
    w = TAU_ * tone / out_rate
    g = abs(alpha / (1 - (1 - alpha) * complex(math.cos(w), -math.sin(w))))
    return TAU_ * dev / 336000 * ampl_conv * g


def test_synthetic_fm_tone_through_the_restatement():
    """Known answer: after the filters settle the audio is a 1 kHz sine (correlation > 0.99) whose amplitude is ampl_conv
    times the per-sample phase step of 75 kHz at 336 kHz times the de-emphasis gain at 1 kHz (within 3 %)."""
    rate, n = 5000000, 131072
    u = fm_tone_u8(rate, 3 * n)
    dec = R.Decoder(1, rate, 48000, 50000, phase="exact")
    audio = np.concatenate([dec.process(u[2 * n * k:2 * n * (k + 1)]) for k in range(3)])
    corr, amp = tone_check(audio)
    assert corr > 0.99, corr
    assert abs(amp / expected_tone_amplitude() - 1) < 0.03, (amp, expected_tone_amplitude())


def test_demod_rejects_bad_arguments_without_a_device():
    L = fsea.hip_lib()
    d = ctypes.c_void_p()
    assert L.fsea_demod_create(None, 1, 5000000, 48000, 1, 0) == FSEA_EINVAL
    for args in ((2, 5000000, 48000, 1), (-1, 5000000, 48000, 1), (1, 0, 48000, 1), (1, 5000000, -5, 1),
                 (1, 5000000, 48000, 0), (1, 5000000, 48000, fsea.DEMOD_MAX_CHANNELS + 1)):
        assert L.fsea_demod_create(ctypes.byref(d), *args, 0) == FSEA_EINVAL, args
        assert not d.value
    assert L.fsea_demod_destroy(None) == 0
    assert L.fsea_demod_reset(None) == FSEA_EINVAL
    assert L.fsea_demod_set_channel(None, 0, 0, 1.0, 0.0) == FSEA_EINVAL
    assert L.fsea_demod_get_channel(None, 0, None, None, None) == FSEA_EINVAL
    assert L.fsea_demod_out_length(None, 131072) == 0
    buf = np.zeros(16, dtype=np.uint8)
    out = np.zeros(16)
    assert L.fsea_demod_u8_host(None, buf.ctypes.data, 8, 0, out.ctypes.data) == FSEA_EINVAL
    assert L.fsea_demod_f64_host(None, out.ctypes.data, out.ctypes.data, 8, out.ctypes.data) == FSEA_EINVAL
    assert L.fsea_demod_u8_device(None, buf.ctypes.data, 8, 0, out.ctypes.data, None) == FSEA_EINVAL


def test_demod_create_without_a_gpu_is_enodevice():
    if fsea.device_count() > 0:
        pytest.skip("a GPU is present")
    L = fsea.hip_lib()
    d = ctypes.c_void_p()
    assert L.fsea_demod_create(ctypes.byref(d), 1, 5000000, 48000, 1, 0) == FSEA_ENODEVICE
    assert not d.value


REF_SRC = "/root/reference/src"


def _members(text, name):
    m = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, text)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    body = re.sub(r"//[^\n]*", "", body)
    return [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]


@pytest.mark.skipif(not os.path.exists(os.path.join(REF_SRC, "nrf.h")), reason="reference tree absent")
def test_reference_members_keep_their_order_and_types():
    ref = open(os.path.join(REF_SRC, "nrf.h")).read()
    ours = open(os.path.join(ROOT, "include", "nrf.h")).read()
    for name in ("nrf_downsampler", "nrf_raw_demodulator", "nrf_fm_demodulator", "nrf_decoder"):
        r, o = _members(ref, name), _members(ours, name)
        assert o[:len(r)] == r, name
        assert all(m.startswith("void *") for m in o[len(r):]), name       # appended backend handles only
    assert re.search(r"NRF_DEMODULATE_RAW = 0,\s*NRF_DEMODULATE_WBFM\s*\}", ours)


def test_reference_members_probe_offsets(tmp_path):
    """The ctypes mirrors in frequensea_amd/nrf.py have the C layout of include/nrf.h."""
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nrf.h"\nint main(void) {\n'
                     'printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(nrf_decoder, freq_shifter), offsetof(nrf_decoder, '
                     'audio_samples), offsetof(nrf_decoder, audio_samples_length), offsetof(nrf_fm_demodulator, '
                     'audio_samples_length), offsetof(nrf_downsampler, out_samples), offsetof(nrf_freq_shifter, cosine));\n'
                     'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [nrf.NrfDecoder.freq_shifter.offset, nrf.NrfDecoder.audio_samples.offset,
                   nrf.NrfDecoder.audio_samples_length.offset, nrf.NrfFmDemodulator.audio_samples_length.offset,
                   nrf.NrfDownsampler.out_samples.offset, nrf.NrfFreqShifter.cosine.offset]


def test_golden_is_small_and_recorded_from_the_fm_capture(gold):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert gold["block__raw"].size == 262144
    assert hashlib.sha256(gold["block__raw"].tobytes()).hexdigest() != hashlib.sha256(bytes(262144)).hexdigest()
