"""Regenerates tests/golden/zoom_golden.npz in the build container only: compiles the reference's own src/nrf.c and
src/nut.c (against the declaration-only stand-in headers of make_iq_filter_golden.py) into a temporary shared library and
records what its frequency shifter followed by its downsampler return -- the chain nrf_decoder runs for its audio, which
the zoom spectrum runs for its rows.  Nothing of the reference is kept but the numbers.

  python tests/golden/make_zoom_golden.py [out.npz]

The input is the committed replay block (tests/golden/rfdata_all_golden.npz: block__raw ^ 0x80, what
nrf_device_get_samples_buffer hands out, N = 131072 pairs).  Per configuration, CALLS consecutive calls on that block:
nrf_freq_shifter_new(SHIFT, in_rate) -> nrf_freq_shifter_process; then nrf_downsampler_new(in_rate, out_rate, out_rate / 2, L)
-> nrf_downsampler_process on the I and on the Q of the first N pairs of the shifter's buffer (its back half stays 0.0).
The rate pairs make rate_mul an exact integer D.  Recorded:
  shift                                   SHIFT, Hz
  zoom__<in>_<out>_<L>__cfg               (D, cutoff, L)
  zoom__<in>_<out>_<L>__taps              nrf_fir_get_low_pass_coefficients(in, cutoff, L): the first L taps
  zoom__<in>_<out>_<L>__len               outputs per call (N // D)
  zoom__<in>_<out>_<L>__idx<k>, __out<k>  call k: the recorded output indices (first / last 256 and 512 between) and the
                                          (I, Q) outputs there
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_demod_golden import subset  # noqa: E402
from make_iq_filter_golden import REF_SRC, build_reference  # noqa: E402  (the same stand-in headers)

GOLDEN = os.path.join(ROOT, "tests", "golden", "zoom_golden.npz")
RATE_PAIRS = [(5000000, 312500), (5000000, 200000), (3000000, 1000000)]   # D = 16, 25, 3
LENGTHS = [41, 97]
SHIFT = 100000
CALLS = 3


def main():
    from frequensea_amd import nrf
    if not os.path.exists(os.path.join(REF_SRC, "nrf.c")):
        sys.exit("needs the reference tree (%s)" % REF_SRC)
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        block = np.ascontiguousarray(z["block__raw"] ^ 0x80)
    n = block.size // 2
    rec = {"shift": np.array(SHIFT)}
    with tempfile.TemporaryDirectory() as tmp:
        L = nrf.bind_demod(nrf.bind_fir(nrf.bind_nut(build_reference(tmp))))
        nrf.bind(L, {name: nrf.API[name] for name in ("nrf_freq_shifter_new", "nrf_freq_shifter_process",
                                                      "nrf_freq_shifter_get_buffer", "nrf_freq_shifter_free")})
        for ci, (rin, rout) in enumerate(RATE_PAIRS):
            for li, length in enumerate(LENGTHS):
                tag = "zoom__%d_%d_%d" % (rin, rout, length)
                cutoff = rout // 2
                p = L.nrf_fir_get_low_pass_coefficients(rin, cutoff, length)
                rec[tag + "__taps"] = np.ctypeslib.as_array(p, shape=(length,)).copy()
                shifter = L.nrf_freq_shifter_new(SHIFT, rin)
                ds_i = L.nrf_downsampler_new(rin, rout, cutoff, length)
                ds_q = L.nrf_downsampler_new(rin, rout, cutoff, length)
                d = ds_i.contents.rate_mul
                assert d == int(d)
                rec[tag + "__cfg"] = np.array([int(d), cutoff, length])
                for k in range(CALLS):
                    buf = L.nut_buffer_new_u8(n, 2, block.ctypes.data)
                    L.nrf_freq_shifter_process(shifter, buf)
                    sb = L.nrf_freq_shifter_get_buffer(shifter)
                    assert sb.contents.length == 2 * n
                    x = nrf.buffer_to_numpy(L, sb).reshape(-1, 2)[:n]
                    out = []
                    for ds, ch in ((ds_i, 0), (ds_q, 1)):
                        samples = np.ascontiguousarray(x[:, ch])
                        L.nrf_downsampler_process(ds, samples.ctypes.data, n)
                        m = ds.contents.out_length
                        out.append(np.ctypeslib.as_array(ds.contents.out_samples, shape=(m,)).copy())
                    assert out[0].size == out[1].size == n // int(d)
                    idx = subset(out[0].size, 100 * ci + 10 * li + k)
                    rec[tag + "__len"] = np.array(out[0].size)
                    rec[tag + "__idx%d" % k] = idx
                    rec[tag + "__out%d" % k] = np.stack([out[0][idx], out[1][idx]], axis=1)
                    L.nut_buffer_free(sb)
                    L.nut_buffer_free(buf)
                L.nrf_downsampler_free(ds_i)
                L.nrf_downsampler_free(ds_q)
                L.nrf_freq_shifter_free(shifter)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(out, **rec)


if __name__ == "__main__":
    main()
