"""Regenerates tests/golden/demod_golden.npz in the build container only: compiles the reference's own src/nrf.c and
src/nut.c (against the declaration-only stand-in headers of make_iq_filter_golden.py) into a temporary shared library and
records what its downsampler, demodulators and decoder return.  Nothing of the reference is kept but the numbers.

  python tests/golden/make_demod_golden.py [out.npz]

Recorded:
  block__raw                  the first 262144-byte replay block of rfdata/rf-100.900-1.raw (the fm-player.lua capture),
                              raw int8 bytes as the file holds them; the decoder reads block__raw ^ 0x80 (device->samples)
  ds__<in>_<out>__*           nrf_downsampler_new(in, out, cutoff, L) over calls of DS_LENGTHS samples in sequence on
                              ds_input(block__raw): __cfg (cutoff, L), per call k __out<k> at the indices __idx<k> (every
                              output of a call of at most SUBSET outputs, else first / last 256 and 512 between) and
                              __len<k>, __sha<k> (sha256 of the whole output, f64 little-endian)
  dm__<raw|wbfm>_<rate>__*    nrf_{raw,fm}_demodulator_new(rate, 48000), three calls on dm_inputs(): __out<k>
  dec__<tag>__*               nrf_decoder_new(type, rate, 48000, offset), three calls on the same block: __out<k> (audio),
                              __pcm<k> ((int16_t)(audio * 32000)), __phase (freq_shifter cosine, sine after each call);
                              tag <wbfm|raw>_<rate>_<offset>, or chg_<rate>: WBFM at 50000, offset 100000 from call 3
"""
import ctypes
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_iq_filter_golden import REF_SRC, build_reference  # noqa: E402  (the same stand-in headers)

GOLDEN = os.path.join(ROOT, "tests", "golden", "demod_golden.npz")
CAPTURE = os.path.join(os.path.dirname(REF_SRC), "rfdata", "rf-100.900-1.raw")
BLOCK = 262144
DS_CONFIGS = [(5000000, 336000, 60000, 51), (10000000, 336000, 60000, 51), (336000, 48000, 10000, 41),
              (5000000, 48000, 24000, 41), (48000, 48000, 24000, 41), (1000000, 3000000, 200000, 41)]
DS_LENGTHS = [1, 7, 50, 4097, 131072]
SUBSET = 1024
DEC_CONFIGS = [(1, 50000), (1, 100000), (1, -120000), (1, 0), (0, 50000)]   # (nrf_demodulate_type, offset)
RATES = [5000000, 10000000]
CALLS = 3


def convert(u8):
    """The reference decoder's conversion of offset-binary bytes: b / 128.0 - 0.995."""
    return u8.astype(np.float64) / 128.0 - 0.995


def ds_input(raw):
    """The downsampler input: converted I samples of the block, then its Q samples."""
    ob = raw ^ 0x80
    return np.concatenate([convert(ob[0::2]), convert(ob[1::2])])


def dm_inputs(raw, captures):
    """The demodulators' three calls (I, Q): the block, a 16384-pair capture, the first 5000 pairs of that capture."""
    out = []
    for r in (raw, captures, captures[:10000]):
        ob = r ^ 0x80
        out.append((convert(ob[0::2]), convert(ob[1::2])))
    return out


def subset(count, seed):
    if count <= SUBSET:
        return np.arange(count, dtype=np.int64)
    rng = np.random.default_rng(seed)
    mid = rng.choice(np.arange(256, count - 256), SUBSET - 512, replace=False)
    return np.unique(np.concatenate([np.arange(256), mid, np.arange(count - 256, count)])).astype(np.int64)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).digest(), dtype=np.uint8)


def pcm(audio):
    return np.trunc(audio * 32000).astype(np.int16)           # (int16_t)(audio * 32000), in range here


def main():
    from frequensea_amd import nrf
    if not os.path.exists(os.path.join(REF_SRC, "nrf.c")):
        sys.exit("needs the reference tree (%s)" % REF_SRC)
    raw = np.fromfile(CAPTURE, dtype=np.uint8, count=BLOCK)
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_golden.npz")) as z:
        capture = z["rf_100p900_1__raw"]
    rec = {"block__raw": raw}
    with tempfile.TemporaryDirectory() as tmp:
        L = nrf.bind_demod(nrf.bind_fir(nrf.bind_nut(build_reference(tmp))))

        x = ds_input(raw)
        for ci, (rin, rout, cutoff, length) in enumerate(DS_CONFIGS):
            tag = "ds__%d_%d" % (rin, rout)
            rec[tag + "__cfg"] = np.array([cutoff, length])
            d = L.nrf_downsampler_new(rin, rout, cutoff, length)
            pos = 0
            for k, n in enumerate(DS_LENGTHS):
                chunk = np.ascontiguousarray(x[pos:pos + n])
                pos += n
                L.nrf_downsampler_process(d, chunk.ctypes.data, n)
                m = d.contents.out_length
                y = np.ctypeslib.as_array(d.contents.out_samples, shape=(m,)).copy() if m else np.zeros(0)
                idx = subset(m, 10 * ci + k)
                rec[tag + "__len%d" % k] = np.array(m)
                rec[tag + "__idx%d" % k] = idx
                rec[tag + "__out%d" % k] = y[idx]
                rec[tag + "__sha%d" % k] = sha(y)
            L.nrf_downsampler_free(d)

        for rate in RATES:
            for kind in ("raw", "wbfm"):
                new = L.nrf_raw_demodulator_new if kind == "raw" else L.nrf_fm_demodulator_new
                proc = L.nrf_raw_demodulator_process if kind == "raw" else L.nrf_fm_demodulator_process
                free = L.nrf_raw_demodulator_free if kind == "raw" else L.nrf_fm_demodulator_free
                dm = new(rate, 48000)
                for k, (i, q) in enumerate(dm_inputs(raw, capture)):
                    i, q = np.ascontiguousarray(i), np.ascontiguousarray(q)
                    proc(dm, i.ctypes.data, q.ctypes.data, i.size)
                    m = dm.contents.audio_samples_length
                    rec["dm__%s_%d__out%d" % (kind, rate, k)] = np.ctypeslib.as_array(dm.contents.audio_samples,
                                                                                       shape=(m,)).copy()
                free(dm)

        samples = np.ascontiguousarray(raw ^ 0x80)
        for rate in RATES:
            runs = [("%s_%d_%d" % ("wbfm" if t else "raw", rate, off), t, off, None) for t, off in DEC_CONFIGS]
            runs.append(("chg_%d" % rate, 1, 50000, 100000))
            for tag, t, off, change in runs:
                dec = L.nrf_decoder_new(t, rate, 48000, off)
                phases = []
                for k in range(CALLS):
                    if change is not None and k == 2:
                        dec.contents.freq_shifter.contents.freq_offset = change
                    L.nrf_decoder_process(dec, samples.ctypes.data, samples.size // 2)
                    m = dec.contents.audio_samples_length
                    a = np.ctypeslib.as_array(dec.contents.audio_samples, shape=(m,)).copy()
                    rec["dec__%s__out%d" % (tag, k)] = a
                    rec["dec__%s__pcm%d" % (tag, k)] = pcm(a)
                    sh = dec.contents.freq_shifter.contents
                    phases.append((sh.cosine, sh.sine))
                rec["dec__%s__phase" % tag] = np.array(phases)
                L.nrf_decoder_free(dec)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(out, **rec)


if __name__ == "__main__":
    main()
