"""Regenerates tests/golden/interp_golden.npz in the build container only.  Nothing of the reference is kept but numbers.

  python tests/golden/make_interp_golden.py [out.npz]

Interpolator: make_iq_draw_golden.py's temporary build of the reference's own src/nrf.c + src/nut.c drives
nrf_interpolator_* on the input sequences of interp_inputs() (committed data), call i passing block i % len(blocks):
  t__<kind>__s<k>                      t after every nrf_interpolator_process call, STEPS[k], CALLS[k] calls
  buf__<kind>__s<k>__calls             the calls after which nrf_interpolator_get_buffer was recorded
  buf__<kind>__s<k>__sha256, __sum     per recorded call: SHA-256 of the payload, its sum (float64)
  buf__<kind>__s<k>__shape             per recorded call: (type, length, channels) of the returned buffer
  buf__<kind>__s<k>__c<call>           the whole payload, for the calls of WHOLE
Movie: the reference's own c/gradual-noise.c, compiled against a declaration-only png.h stand-in whose png_write_png
appends the frame's rows to a file and ends the process after MOVIE_FRAMES frames, run in a temporary directory on the
capture files of movie_captures().  So the movie frames are pinned to the reference's binary, not to a restatement.
  movie__sha256                        per frame 1...MOVIE_FRAMES: SHA-256 of the 1920 x 1080 bytes
  movie__rowsum, movie__colsum         per frame of MOVIE_SUMS: row and column sums (int64)
  movie__frame<n>                      frame MOVIE_WHOLE itself (it deflates to a few per cent)
"""
import ctypes
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "tests", "golden")
GOLDEN = os.path.join(HERE, "interp_golden.npz")
REF_C = "/root/reference/c"

STEPS = [0.01, 0.3, 1.0]
CALLS = [210, 14, 7]
RECORDED = [[0, 1, 50, 100, 101, 102, 150, 201, 202, 203], list(range(14)), list(range(7))]
WHOLE = {("u8", 0): [100, 102], ("f64", 0): [100, 101], ("f64", 1): [4], ("f64", 2): [1]}
MOVIE_FRAMES = 205
MOVIE_SUMS = [1, 2, 50, 100, 101, 150, 200, 201, 205]
MOVIE_WHOLE = 50
MOVIE_W, MOVIE_H = 1920, 1080

PNG_H = """
#include <stdint.h>
#include <stdio.h>
typedef struct png_stub *png_structp;
typedef struct png_stub *png_infop;
typedef unsigned char *png_bytep;
typedef png_bytep *png_bytepp;
#define PNG_LIBPNG_VER_STRING "stub"
#define PNG_COLOR_TYPE_GRAY 0
#define PNG_INTERLACE_NONE 0
#define PNG_COMPRESSION_TYPE_DEFAULT 0
#define PNG_FILTER_TYPE_DEFAULT 0
#define PNG_TRANSFORM_IDENTITY 0
png_structp png_create_write_struct(const char *v, void *a, void *b, void *c);
png_infop png_create_info_struct(png_structp p);
void png_destroy_write_struct(png_structp *p, png_infop *i);
void png_set_IHDR(png_structp p, png_infop i, int w, int h, int d, int c, int il, int ct, int ft);
void *png_malloc(png_structp p, size_t n);
void png_free(png_structp p, void *m);
void png_init_io(png_structp p, FILE *fp);
void png_set_rows(png_structp p, png_infop i, png_bytepp rows);
void png_write_png(png_structp p, png_infop i, int t, void *x);
"""

PNG_C = """
#include <stdlib.h>
#include "png.h"
struct png_stub { int w, h; png_bytepp rows; };
static struct png_stub one;
static int frames;
png_structp png_create_write_struct(const char *v, void *a, void *b, void *c) { (void)v; (void)a; (void)b; (void)c; return &one; }
png_infop png_create_info_struct(png_structp p) { return p; }
void png_destroy_write_struct(png_structp *p, png_infop *i) { (void)p; (void)i; }
void png_set_IHDR(png_structp p, png_infop i, int w, int h, int d, int c, int il, int ct, int ft) {
    (void)i; (void)d; (void)c; (void)il; (void)ct; (void)ft; p->w = w; p->h = h;
}
void *png_malloc(png_structp p, size_t n) { (void)p; return malloc(n); }
void png_free(png_structp p, void *m) { (void)p; free(m); }
void png_init_io(png_structp p, FILE *fp) { (void)p; (void)fp; }
void png_set_rows(png_structp p, png_infop i, png_bytepp rows) { (void)i; p->rows = rows; }
void png_write_png(png_structp p, png_infop i, int t, void *x) {
    (void)i; (void)t; (void)x;
    FILE *out = fopen(getenv("STUB_FRAMES"), "ab");
    for (int y = 0; y < p->h; y++) fwrite(p->rows[y], 1, (size_t)p->w, out);
    fclose(out);
    if (++frames >= atoi(getenv("STUB_MAX_FRAMES"))) exit(0);
}
"""


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def interp_inputs():
    """kind -> (blocks, length, channels): the committed data the interpolator sequences are built from.
    u8: three 262144-byte blocks (the replay block, its reverse, sixteen 16384-byte captures), offset binary.
    f64: four blocks of 10239 doubles (recorded nrf_iq_filter outputs), one channel: 81912 bytes, no multiple of 16."""
    with np.load(os.path.join(HERE, "rfdata_all_golden.npz")) as z:
        block = z["block__raw"]
        caps = [z[k] for k in sorted(z.files) if k.endswith("__raw") and k.startswith("rf_")][:16]
    u8 = np.stack([block, block[::-1], np.concatenate(caps)]).astype(np.uint8) ^ np.uint8(0x80)
    with np.load(os.path.join(HERE, "iq_filter_golden.npz")) as z:
        f64 = np.concatenate([z["iq__200000_51__out"].reshape(3, -1), z["dvbt__out"].reshape(3, -1)[:1]])[:, :10239]
    return {"u8": (np.ascontiguousarray(u8), 131072, 2), "f64": (np.ascontiguousarray(f64), 10239, 1)}


def movie_captures():
    """The four capture files of the movie run, 131072 raw bytes each, for 1.000, 1.010, 1.020 and 1.030 MHz."""
    raw = interp_inputs()["u8"][0] ^ np.uint8(0x80)
    caps = [raw[0][:131072], raw[1][:131072], raw[2][:131072], raw[0][131072:]]
    # the ends of the byte range meet in the first eight samples of every pair, so that the clamp and the truncation are
    # hit at both ends
    ends = [np.array([0, 255, 127, 128, 0, 255, 0, 255], dtype=np.uint8), np.array([255, 0, 128, 127, 0, 255, 127, 128], dtype=np.uint8)]
    caps = [c.copy() for c in caps]
    for k, c in enumerate(caps):
        c[0:16:2] = ends[k % 2] ^ np.uint8(0x80)
    return [np.ascontiguousarray(c) for c in caps]


def movie_frames(tmp):
    """Frames 1...MOVIE_FRAMES of the reference's gradual-noise binary on movie_captures(), (MOVIE_FRAMES, H, W) uint8."""
    os.makedirs(os.path.join(tmp, "stub"))
    os.makedirs(os.path.join(tmp, "rftmp"))
    os.makedirs(os.path.join(tmp, "run", "_export"))
    with open(os.path.join(tmp, "stub", "png.h"), "w") as fp:
        fp.write(PNG_H)
    with open(os.path.join(tmp, "png_stub.c"), "w") as fp:
        fp.write(PNG_C)
    exe = os.path.join(tmp, "gradual-noise")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-w", "-I" + os.path.join(tmp, "stub"), "-I" + REF_C,
                    os.path.join(REF_C, "gradual-noise.c"), os.path.join(tmp, "png_stub.c"), "-o", exe, "-lm"], check=True)
    for k, c in enumerate(movie_captures()):
        c.tofile(os.path.join(tmp, "rftmp", "rf-%.3f-big.raw" % (1.0 + 0.01 * k)))
    frames = os.path.join(tmp, "frames.bin")
    subprocess.run([exe], cwd=os.path.join(tmp, "run"), check=True, stdout=subprocess.DEVNULL,
                   env=dict(os.environ, STUB_FRAMES=frames, STUB_MAX_FRAMES=str(MOVIE_FRAMES)))
    return np.fromfile(frames, dtype=np.uint8).reshape(MOVIE_FRAMES, MOVIE_H, MOVIE_W)


def main():
    from frequensea_amd import nrf
    draw = _load("make_iq_draw_golden")
    gen = draw._load_filter_generator()
    if not os.path.exists(os.path.join(gen.REF_SRC, "nrf.c")):
        sys.exit("needs the reference tree (%s)" % gen.REF_SRC)
    rec = {"steps": np.array(STEPS), "calls": np.array(CALLS)}
    with tempfile.TemporaryDirectory() as tmp:
        L = nrf.bind_interpolator(nrf.bind_nut(draw.build_reference(gen, tmp)))
        for kind, (blocks, length, channels) in interp_inputs().items():
            new = L.nut_buffer_new_u8 if kind == "u8" else L.nut_buffer_new_f64
            for k, (step, calls) in enumerate(zip(STEPS, CALLS)):
                key = "%s__s%d" % (kind, k)
                ip = L.nrf_interpolator_new(step)
                assert ip.contents.t == -1.0
                ts, shas, sums, shapes = [], [], [], []
                for i in range(calls):
                    b = blocks[i % len(blocks)]
                    buf = new(length, channels, b.ctypes.data)
                    L.nrf_interpolator_process(ip, buf)
                    L.nut_buffer_free(buf)
                    ts.append(ip.contents.t)
                    if i in RECORDED[k]:
                        got = L.nrf_interpolator_get_buffer(ip)
                        c = got.contents
                        shapes.append((c.type, c.length, c.channels))
                        a = nrf.buffer_to_numpy(L, got)
                        L.nut_buffer_free(got)
                        shas.append(sha(a))
                        sums.append(float(a.astype(np.float64).sum()))
                        if i in WHOLE.get((kind, k), []):
                            rec["buf__%s__c%d" % (key, i)] = a
                L.nrf_interpolator_free(ip)
                rec["t__" + key] = np.array(ts)
                rec["buf__%s__calls" % key] = np.array(RECORDED[k])
                rec["buf__%s__sha256" % key] = np.stack(shas)
                rec["buf__%s__sum" % key] = np.array(sums)
                rec["buf__%s__shape" % key] = np.array(shapes)
    with tempfile.TemporaryDirectory() as tmp:
        frames = movie_frames(tmp)
        rec["movie__sha256"] = np.stack([sha(f) for f in frames])
        rec["movie__sums_of"] = np.array(MOVIE_SUMS)
        rec["movie__rowsum"] = np.stack([frames[n - 1].astype(np.int64).sum(axis=1) for n in MOVIE_SUMS])
        rec["movie__colsum"] = np.stack([frames[n - 1].astype(np.int64).sum(axis=0) for n in MOVIE_SUMS])
        rec["movie__frame%d" % MOVIE_WHOLE] = frames[MOVIE_WHOLE - 1].copy()
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(out, **rec)


if __name__ == "__main__":
    main()
