"""Regenerates tests/golden/trace_golden.npz in the build container only.  Nothing of the reference is kept but numbers.

  python tests/golden/make_trace_golden.py [out.npz]

The reference's own c/single-sample.c is compiled in a temporary directory against make_interp_golden.py's declaration-only
png.h stand-in, whose png_write_png appends every frame's rows to a file, and run on the inputs of cases() (built from
committed data).  So the frames are pinned to the reference's binary, not to a restatement.  Per case <c> of CASES:
  <c>__args                 the tool's -s, -f, -p and whether -v was given
  <c>__sha256               per written frame: SHA-256 of the 1920 x 1080 bytes (with -v: the one image the tool writes)
  <c>__sums_of, __rowsum, __colsum   row and column sums (int64) of a few frames
  <c>__frame<n>             whole frames (they deflate to little)
Every case but "odd" keeps the reference inside its buffer (-s even and a divisor of the size).  In "odd" the last point of
the last frame takes its Q byte from behind the buffer: that frame is recorded like the others and no test compares it.
"""
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
GOLDEN = os.path.join(HERE, "trace_golden.npz")
REF_C = os.environ.get("FSEA_REFERENCE_C", os.path.join(os.path.dirname(ROOT), "reference", "c"))
W, H = 1920, 1080

# name: (input, -s, -f, -p, -v, frames whose sums are kept, whole frames kept)
CASES = {
    "defaults": ("block", 100, 0, 4, False, [1, 2, 100, 200], [200]),
    "fade": ("long", 1024, 3, 40, False, [1, 8, 16], [2]),
    "two": ("long", 4096, 0, 100, False, [1, 4], []),
    "preview": ("long", 1024, 3, 40, True, [1], []),
    "odd": ("long_odd", 333, 1, 30, False, [1, 24, 47], []),
}


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def inputs():
    """The capture files of the cases, raw int8 bytes as a HackRF writes them.
    block: the first 20000 bytes of the committed replay block.
    long: 16384 bytes of it spread over the whole byte range (times 37 modulo 256), so that the lines are long; every
          frame of 1024 bytes starts with the same eight points (their segments are hit again and again: saturation), and
          points on the x == 0 and y == 0 borders of the IQ square are put in (byte 128 is coordinate 0).
    long_odd: the first 48 * 333 bytes of `long`."""
    with np.load(os.path.join(HERE, "rfdata_all_golden.npz")) as z:
        block = np.ascontiguousarray(z["block__raw"]).view(np.uint8)
    long = (block[20000:20000 + 16384].astype(np.uint32) * 37 % 256).astype(np.uint8)
    for j in range(0, 16384, 1024):
        long[j:j + 16] = long[0:16]
    long[40:48] = [128, 7, 128, 200, 90, 128, 255, 128]      # (0, 135), (0, 72), (218, 0), (127, 0)
    long[5000:5004] = [128, 128, 127, 127]                   # (0, 0) to (255, 255)
    return {"block": block[:20000].copy(), "long": long, "long_odd": long[:48 * 333].copy()}


def build_reference(tmp):
    stub = _load("make_interp_golden")
    os.makedirs(os.path.join(tmp, "stub"))
    with open(os.path.join(tmp, "stub", "png.h"), "w") as fp:
        fp.write(stub.PNG_H)
    with open(os.path.join(tmp, "png_stub.c"), "w") as fp:
        fp.write(stub.PNG_C)
    exe = os.path.join(tmp, "single-sample")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-w", "-I" + os.path.join(tmp, "stub"), "-I" + REF_C,
                    os.path.join(REF_C, "single-sample.c"), os.path.join(tmp, "png_stub.c"), "-o", exe, "-lm"], check=True)
    return exe


def reference_frames(exe, tmp, data, s, f, p, preview):
    """What the reference's binary writes for one capture, (frames, H, W) uint8."""
    run = tempfile.mkdtemp(dir=tmp)
    os.makedirs(os.path.join(run, "_export"))
    data.tofile(os.path.join(run, "capture.raw"))
    frames = os.path.join(run, "frames.bin")
    args = [exe, "-s", str(s), "-f", str(f), "-p", str(p)] + (["-v"] if preview else []) + ["capture.raw"]
    subprocess.run(args, cwd=run, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                   env=dict(os.environ, STUB_FRAMES=frames, STUB_MAX_FRAMES="1000000"))
    out = np.fromfile(frames, dtype=np.uint8).reshape(-1, H, W)
    os.remove(frames)
    return out


def main():
    if not os.path.exists(os.path.join(REF_C, "single-sample.c")):
        sys.exit("needs the reference tree (%s)" % REF_C)
    rec = {}
    data = inputs()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(tmp)
        for name, (inp, s, f, p, preview, sums_of, whole) in CASES.items():
            frames = reference_frames(exe, tmp, data[inp], s, f, p, preview)
            n = -(-data[inp].size // s)
            assert len(frames) == (1 if preview else n), (name, len(frames))
            if name in ("fade", "two"):
                # saturation: some pixel stands where the next hit is refused
                assert int(frames.max()) + p >= 255, (name, int(frames.max()))
            if name == "two":
                assert int(frames.max()) == 200
            rec[name + "__args"] = np.array([s, f, p, int(preview)])
            rec[name + "__sha256"] = np.stack([sha(fr) for fr in frames])
            rec[name + "__sums_of"] = np.array(sums_of)
            rec[name + "__rowsum"] = np.stack([frames[k - 1].astype(np.int64).sum(axis=1) for k in sums_of])
            rec[name + "__colsum"] = np.stack([frames[k - 1].astype(np.int64).sum(axis=0) for k in sums_of])
            for k in whole:
                rec["%s__frame%d" % (name, k)] = frames[k - 1].copy()
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(out, **rec)


if __name__ == "__main__":
    main()
