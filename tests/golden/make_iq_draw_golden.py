"""Regenerates tests/golden/iq_draw_golden.npz in the build container only: compiles the reference's own src/nrf.c and
src/nut.c (with the declaration-only header stand-ins of make_iq_filter_golden.py, plus radio entry points that report "no
device" so that nrf_device_new falls back on its replay file) into a temporary shared library and records what its IQ
drawing functions and signal detector return.  Nothing of the reference is kept but the numbers.

  python tests/golden/make_iq_draw_golden.py [out.npz]

Inputs (all from committed data, see iq_inputs()):
  block       the replay device's block (rfdata_all_golden.npz block__raw ^ 0x80), U8, 131072 pairs
  filt51      nrf_iq_filter_new(5e6, 200e3, 51) outputs recorded in iq_filter_golden.npz (three steps, concatenated), F64
  filt97      the same for (60e3, 97)
  dvbt        the dvbt.lua shifter -> filter outputs recorded there (half of the points from the zero back half), F64
  synthetic   F64 values around and far outside [0, 1), NaN and infinities (in__synthetic)
Recorded per input <name>:
  points__<name>                         nrf_buffer_to_iq_points, 65536 bytes
  lines__<name>__m<m>__p<k>__sha256      nrf_buffer_to_iq_lines(buf, m, PCTS[k]) for m in 1, 2, 4: SHA-256 of the image,
  lines__<name>__m<m>__p<k>__rowsum      its row sums (int64), and for m = 1 the image itself (__image)
  coords__synthetic                      nut_buffer_get_u8 of every element of in__synthetic
Device (a paused replay device on replay_file(): three blocks, stepped through twice):
  device__points, device__lines_sha256, device__lines_rowsum
                                         per block of the file: nrf_device_get_iq_buffer, nrf_device_get_iq_lines(dev,
                                         DEVICE_M, DEVICE_PCT) while the device rests on it
Host:
  position__u8_in / __u8_out, position__f64_in / __f64_out   nrf_buffer_add_position_channel (U8 2 channels, F64 3)
  detector__<name>                       nrf_signal_detector_process: (mean, standard_deviation) on filt51 and block
"""
import ctypes
import hashlib
import importlib.util
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "tests", "golden")
GOLDEN = os.path.join(HERE, "iq_draw_golden.npz")

PCTS = np.array([0.0, 0.2, 0.3, 1.0, 1.5, -0.25, np.nan], dtype=np.float32)
MULTIPLIERS = [1, 2, 4]
DEVICE_M, DEVICE_PCT = 2, 0.3
DEVICE_STEPS = 6
SPECIALS = [-0.01, -0.001, 1.0, 1.004, 1.5, -1.5, np.nan, np.inf, -np.inf, 1e10, -1e10, 8388607.99, 8388608.0,
            -8388608.0, -8388608.004, 0.5, 0.999, 255 / 256, 1 / 256, -1 / 256, 2.0 - 1e-12, 1e300, -0.0]

# the radio entry points nrf_device_new tries first: no RTL-SDR, HackRF initialises but opens nothing
RADIO_STUBS = """
typedef struct rtlsdr_dev rtlsdr_dev_t;
typedef struct hackrf_device hackrf_device;
int rtlsdr_open(rtlsdr_dev_t **dev, unsigned int index) { (void)dev; (void)index; return -1; }
int hackrf_init(void) { return 0; }
int hackrf_open(hackrf_device **device) { (void)device; return -1; }
int hackrf_exit(void) { return 0; }
"""


def _load_filter_generator():
    spec = importlib.util.spec_from_file_location("make_iq_filter_golden", os.path.join(HERE, "make_iq_filter_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_reference(gen, tmp):
    """make_iq_filter_golden.py's build of the reference's nrf.c + nut.c, with the radio stubs linked in."""
    import subprocess
    for name, text in gen.STUBS.items():
        path = os.path.join(tmp, "stub", name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fp:
            fp.write(text)
    stub_c = os.path.join(tmp, "radio_stubs.c")
    with open(stub_c, "w") as fp:
        fp.write(RADIO_STUBS)
    so = os.path.join(tmp, "ref_nrf.so")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-shared", "-w", "-Wno-error=implicit-function-declaration",
                    "-I" + os.path.join(tmp, "stub"), "-I" + gen.REF_SRC, os.path.join(gen.REF_SRC, "nrf.c"),
                    os.path.join(gen.REF_SRC, "nut.c"), stub_c, "-o", so, "-lm", "-lpthread"], check=True)
    return ctypes.CDLL(so, mode=os.RTLD_LAZY)


def sha(img):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(img).tobytes()).digest(), dtype=np.uint8)


def rowsum(img, m):
    return np.asarray(img, dtype=np.int64).reshape(256 * m, 256 * m).sum(axis=1)


def iq_inputs():
    """name -> interleaved IQ (uint8 or float64), the committed data the golden images are drawn from."""
    with np.load(os.path.join(HERE, "rfdata_all_golden.npz")) as z:
        block = np.ascontiguousarray(z["block__raw"] ^ 0x80)
    with np.load(os.path.join(HERE, "iq_filter_golden.npz")) as z:
        filt51 = np.ascontiguousarray(z["iq__200000_51__out"].reshape(-1))
        filt97 = np.ascontiguousarray(z["iq__60000_97__out"].reshape(-1))
        dvbt = np.ascontiguousarray(z["dvbt__out"].reshape(-1))
    return {"block": block, "filt51": filt51, "filt97": filt97, "dvbt": dvbt, "synthetic": synthetic()}


def synthetic():
    """4096 pairs: the special values, each beside every other one, then a ramp over [-3, 3)."""
    s = np.array(SPECIALS, dtype=np.float64)
    pairs = np.stack(np.meshgrid(s, s, indexing="ij"), axis=-1).reshape(-1)
    ramp = np.linspace(-3.0, 3.0, 2 * 4096 - pairs.size, endpoint=False)
    return np.ascontiguousarray(np.concatenate([pairs, ramp]))


def replay_file(path):
    """Three blocks: the golden block, the same bytes reversed, and sixteen 16384-byte captures."""
    with np.load(os.path.join(HERE, "rfdata_all_golden.npz")) as z:
        block = z["block__raw"]
        caps = [z[k] for k in sorted(z.files) if k.endswith("__raw") and k.startswith("rf_")][:16]
    data = np.concatenate([block, block[::-1], np.concatenate(caps)]).astype(np.uint8)
    assert data.size == 3 * 262144
    data.tofile(path)
    return data.reshape(3, -1)


def to_nut(L, nrf, a):
    if a.dtype == np.uint8:
        return L.nut_buffer_new_u8(a.size // 2, 2, a.ctypes.data)
    return L.nut_buffer_new_f64(a.size // 2, 2, a.ctypes.data)


def main():
    from frequensea_amd import nrf
    gen = _load_filter_generator()
    if not os.path.exists(os.path.join(gen.REF_SRC, "nrf.c")):
        sys.exit("needs the reference tree (%s)" % gen.REF_SRC)
    rec = {"lines__pcts": PCTS, "lines__multipliers": np.array(MULTIPLIERS)}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_reference(gen, tmp)
        nrf.bind_iq_draw(nrf.bind_nut(L))
        vp = ctypes.c_void_p
        nrf.bind(L, {name: nrf.API[name] for name in (
                    "nrf_device_new", "nrf_device_set_paused", "nrf_device_step",
                    "nrf_device_get_samples_buffer", "nrf_device_free")})

        def take(buf):
            out = nrf.buffer_to_numpy(L, buf)
            L.nut_buffer_free(buf)
            return out

        inputs = iq_inputs()
        rec["in__synthetic"] = inputs["synthetic"]
        for name, a in inputs.items():
            buf = to_nut(L, nrf, a)
            rec["points__" + name] = take(L.nrf_buffer_to_iq_points(buf))
            for m in MULTIPLIERS:
                for k, p in enumerate(PCTS):
                    img = take(L.nrf_buffer_to_iq_lines(buf, m, float(p)))
                    assert img.size == (256 * m) ** 2
                    key = "lines__%s__m%d__p%d" % (name, m, k)
                    rec[key + "__sha256"] = sha(img)
                    rec[key + "__rowsum"] = rowsum(img, m)
                    if m == 1:
                        rec[key + "__image"] = img
            if name == "synthetic":
                rec["coords__synthetic"] = np.array([L.nut_buffer_get_u8(buf, i) for i in range(a.size)], np.uint8)
            L.nut_buffer_free(buf)

        # the replay device, paused, stepped through its three blocks twice
        path = os.path.join(tmp, "replay.raw")
        blocks = replay_file(path) ^ np.uint8(0x80)
        dev = L.nrf_device_new(100.0, path.encode())
        L.nrf_device_set_paused(dev, 1)
        per_block = {}
        for step in range(DEVICE_STEPS):
            time.sleep(0.1)                     # > 2 replay periods: the current block has been ingested
            s = take(L.nrf_device_get_samples_buffer(dev))
            match = [b for b in range(3) if np.array_equal(s, blocks[b])]
            assert len(match) == 1, step
            img = take(L.nrf_device_get_iq_lines(dev, DEVICE_M, DEVICE_PCT))
            got = (take(L.nrf_device_get_iq_buffer(dev)), sha(img), rowsum(img, DEVICE_M))
            if match[0] in per_block:           # the second visit of a block draws the same images
                assert all(np.array_equal(a, b) for a, b in zip(per_block[match[0]], got)), step
            per_block[match[0]] = got
            L.nrf_device_step(dev)
        L.nrf_device_free(dev)
        assert sorted(per_block) == [0, 1, 2]
        rec["device__points"] = np.stack([per_block[b][0] for b in range(3)])
        rec["device__lines_sha256"] = np.stack([per_block[b][1] for b in range(3)])
        rec["device__lines_rowsum"] = np.stack([per_block[b][2] for b in range(3)])

        # add_position_channel on a U8 and an F64 buffer (F64 with 3 channels: the pairs are read across them)
        u8_in = np.ascontiguousarray(inputs["block"][:2 * 4096])
        buf = L.nut_buffer_new_u8(4096, 2, u8_in.ctypes.data)
        rec["position__u8_in"], rec["position__u8_out"] = u8_in, take(L.nrf_buffer_add_position_channel(buf))
        L.nut_buffer_free(buf)
        f_in = np.ascontiguousarray(inputs["filt51"][:3 * 1000])
        buf = L.nut_buffer_new_f64(1000, 3, f_in.ctypes.data)
        rec["position__f64_in"], rec["position__f64_out"] = f_in, take(L.nrf_buffer_add_position_channel(buf))
        L.nut_buffer_free(buf)

        # the signal detector on the filtered block and on the raw one
        for name in ("filt51", "block"):
            det = L.nrf_signal_detector_new()
            buf = to_nut(L, nrf, inputs[name])
            L.nrf_signal_detector_process(det, buf)
            rec["detector__" + name] = np.array([det.contents.mean, det.contents.standard_deviation])
            L.nut_buffer_free(buf)
            L.nrf_signal_detector_free(det)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(out, **rec)


if __name__ == "__main__":
    main()
