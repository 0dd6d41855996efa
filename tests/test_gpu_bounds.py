"""GPU tier: every device form that writes through a caller's pointer, once between guard bands at its smallest ragged
shapes, and every input once between two different fills (tests/guarded.py).

The value tests of the other files cannot see a kernel that stores a few elements outside the buffer it was given (the
allocator rounds an exact-sized buffer up, the host forms' staging has slack), nor one whose result depends on bytes behind
the n samples it was given.  Here
  - every output is a Guarded payload of exactly the documented size, 64 KiB of 0xA5 in front of and behind it (and in it:
    an element that should have been written and was not shows too); after the call both bands are as they were and the
    payload equals the family's oracle;
  - every input is a Guarded payload of exactly its n samples and the call runs twice on objects in a fresh state, the
    input's bands 0x00 the first time and 0xFF the second (f32 / f64 inputs: 0.0 and a NaN).  Both runs equal the oracle bit
    for bit, so they equal each other; short follow-up calls on the same objects (5 samples, and one decimation step where 5
    samples give no output) show that the carried tail, phase and state took nothing from behind the input either.
Oracles: the host form of another object in a fresh state, bit for bit, wherever the host form queues the same launches (it
does in every family: each fsea_*_host runs the launch function of its device form through the object's staging); beside it
the numpy restatements the family's own test file imports (points_image / lines_image, persist_ref, numpy_sums, trace_ref,
interp_ref).  No tolerance appears here: every comparison is of bytes.  A fresh state is a new object or reset(), which
include/fsea.h defines as one.
The one exception to "bands stay clean" is test_the_bands_catch_a_store_one_sample_past_the_payload."""
import numpy as np
import pytest

from frequensea_amd import fsea
from tests import interp_ref, persist_ref, trace_ref
from tests.guarded import FILL, GUARD, Guarded
from tests.test_gpu_fir import random_taps
from tests.test_gpu_iq_draw import lines_image, points_image
from tests.test_gpu_signal_capture import numpy_sums
from tests.test_gpu_zoom import lowpass_like_taps
from tests.test_iq_draw_host import GOLDEN as IQ_GOLDEN

pytestmark = pytest.mark.gpu

INPUT_FILLS = (0x00, 0xFF)          # the bands round an input: zeros / 0.0, then 0xFF / a NaN
CPS, PHASE0, OFFSET = -1.2e6 / 10e6, 0.3, 1234563      # the shifted forms; the offset is no multiple of 8
FOLLOW_UP = 5                       # samples of the short call behind each one


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, "first difference at byte %d of %d" % (
        int(np.flatnonzero(got.view(np.uint8).ravel() != want.view(np.uint8).ravel())[0]), got.nbytes))


def fenced(arr, fill, lead=0):
    """A host array as a device input of exactly its bytes, `lead` bytes behind a 16-byte boundary, the bands (and the lead)
    holding `fill`: (the Guarded, the device address of the data)."""
    arr = np.ascontiguousarray(arr)
    g = Guarded(lead + arr.nbytes, fill=fill).upload(arr, lead)
    return g, g.addr + lead


class Outputs:
    """The guarded outputs of one call, by name: .addr(name), and .take(name, dtype, shape) checks the bands and returns the
    payload; .free() them all."""

    def __init__(self, **nbytes):
        self.g = {k: Guarded(v) for k, v in nbytes.items()}

    def addr(self, name):
        return self.g[name].addr

    def take(self, name, dtype, shape, what):
        self.g[name].check((what, name))
        return self.g[name].payload(dtype, shape)

    def free(self):
        for g in self.g.values():
            g.free()


# ---- the filter -----------------------------------------------------------------------------------------------------

FIR_COUNTS = [1, 2, 3, 2047, 2048, 2049, 4097]      # pair and single stores at the end of one, two and three tiles


def fir_device(fir, shifted, d_in, n, d_out, flip, consumed=0):
    if shifted:
        fir.run_shifted_device(d_in, n, d_out, CPS, PHASE0, OFFSET + consumed, flip=flip)
    else:
        fir.run_device(d_in, n, d_out, flip=flip)


def fir_host(fir, shifted, iq, flip, consumed=0):
    return fir.run_u8_shifted(iq, CPS, PHASE0, OFFSET + consumed, flip=flip) if shifted else fir.run_u8(iq, flip=flip)


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("L", [1, 51, fsea.FIR_MAX_TAPS])
def test_fir(L, flip, shifted):
    c = random_taps(L, L)
    rng = np.random.default_rng(10 * L + 2 * flip + shifted)
    oracle, firs = fsea.Fir(c), [fsea.Fir(c) for _ in INPUT_FILLS]
    for n in FIR_COUNTS:
        iq, more = rng.integers(0, 256, 2 * n, dtype=np.uint8), rng.integers(0, 256, 2 * FOLLOW_UP, dtype=np.uint8)
        oracle.reset()
        want = fir_host(oracle, shifted, iq, flip)
        want_more = fir_host(oracle, shifted, more, flip, n)
        for fir, fill in zip(firs, INPUT_FILLS):
            what = (L, flip, shifted, n, fill)
            fir.reset()
            (g_in, d_in), (g_more, d_more) = fenced(iq, fill), fenced(more, fill)
            out = Outputs(y=8 * n, more=8 * FOLLOW_UP)
            fir_device(fir, shifted, d_in, n, out.addr("y"), flip)
            fir_device(fir, shifted, d_more, FOLLOW_UP, out.addr("more"), flip, n)
            same(out.take("y", np.complex64, n, what), want, what)
            same(out.take("more", np.complex64, FOLLOW_UP, what), want_more, (what, "follow-up"))
            g_in.check((what, "input")), g_more.check((what, "input of the follow-up"))
            g_in.free(), g_more.free(), out.free()
    for f in [oracle] + firs:
        f.close()


def test_the_bands_catch_a_store_one_sample_past_the_payload():
    """The harness bites: n + 1 samples asked for into a payload of n, n even, so the extra sample is the single store of
    fir_body's odd tail.  Its 8 bytes land in the back band, memory this test owns, at offsets 0 .. 7.  The only test that
    expects a dirty band."""
    n, c = 2, random_taps(51, 51)
    iq = np.full(2 * (n + 1), 255, np.uint8)
    fir = fsea.Fir(c)
    want = fir.run_u8(iq)
    stray = np.flatnonzero(want[n:].view(np.uint8) != FILL)     # (a byte that equals the fill would not show)
    assert stray.size >= 6
    fir.reset()
    g_in, d_in = fenced(iq, FILL)
    out = Guarded(8 * n)
    fir.run_device(d_in, n + 1, out.addr)
    found = out.dirty()
    assert found == [("back", int(stray[0]), int(stray[-1]), stray.size)] and 0 <= stray[0] <= stray[-1] <= 7, found
    with pytest.raises(AssertionError, match=r"back band: %d bytes changed, offsets %d\.\.%d" % (stray.size, stray[0], stray[-1])):
        out.check("n + 1 samples into a payload of n")
    same(out.payload(np.complex64, n), want[:n], "the payload itself")
    g_in.free(), out.free(), fir.close()


# ---- the chain ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lines_m", [1, 3])
@pytest.mark.parametrize("stage", ["unshifted", "n_zero 0", "n_zero 7"])
@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("n", [1, 2049])
def test_chain(n, n_frames, stage, lines_m):
    """Points, lines and pairs together, per frame, against n_frames single host runs of another chain.  Frames with zero
    samples need n_samples a multiple of 8 and n_zero even (include/fsea.h): with n_zero = 7 and three frames the call is
    refused, and must then have written nothing."""
    c = fsea.lowpass_taps(5e6, 200e3, 51)
    shifted, n_zero = stage != "unshifted", 7 if stage == "n_zero 7" else 0
    per, m2 = n + n_zero, (256 * lines_m) ** 2
    rng = np.random.default_rng(n + n_frames + lines_m)
    iq, more = rng.integers(0, 256, 2 * n * n_frames, dtype=np.uint8), rng.integers(0, 256, 2 * FOLLOW_UP, dtype=np.uint8)

    def st(consumed, zeros):
        return fsea.Chain.stage(flip=True, cycles_per_sample=CPS, phase0_cycles=PHASE0, sample_offset=OFFSET + consumed,
                                n_zero=zeros) if shifted else fsea.Chain.stage(flip=True)

    refused = n_frames > 1 and n_zero
    if not refused:
        single = fsea.Chain(c)
        want = [single.run(iq[2 * n * f:2 * n * (f + 1)], st(f * n, n_zero), points=True, lines_m=lines_m, pairs=True)
                for f in range(n_frames)]
        want_more = single.run(more, st(n_frames * n, 0), points=True, lines_m=lines_m, pairs=True)
        single.close()
    for fill in INPUT_FILLS:
        what = (n, n_frames, stage, lines_m, fill)
        chain = fsea.Chain(c)
        (g_in, d_in), (g_more, d_more) = fenced(iq, fill), fenced(more, fill)
        out = Outputs(points=65536 * n_frames, lines=m2 * n_frames, pairs=8 * per * n_frames)
        run = lambda: chain.run_device(d_in, n, n_frames, st(0, n_zero), d_points=out.addr("points"), d_lines=out.addr("lines"),
                                       lines_m=lines_m, d_pairs=out.addr("pairs"))
        if refused:
            with pytest.raises(fsea.FseaError):
                run()
            for name, g in out.g.items():
                g.check((what, name))
                assert np.all(g.payload(np.uint8, g.nbytes) == FILL), (what, name)
        else:
            run()
            pts = out.take("points", np.uint8, (n_frames, 256, 256), what)
            lns = out.take("lines", np.uint8, (n_frames, 256 * lines_m, 256 * lines_m), what)
            prs = out.take("pairs", np.complex64, (n_frames, per), what)
            for f in range(n_frames):
                same(prs[f], want[f]["pairs"], (what, f, "pairs"))
                same(pts[f], want[f]["points"], (what, f, "points"))
                same(lns[f], want[f]["lines"], (what, f, "lines"))
            assert chain.n_pairs == per
            nxt = Outputs(points=65536, lines=m2, pairs=8 * FOLLOW_UP)
            chain.run_device(d_more, FOLLOW_UP, 1, st(n_frames * n, 0), d_points=nxt.addr("points"), d_lines=nxt.addr("lines"),
                             lines_m=lines_m, d_pairs=nxt.addr("pairs"))
            same(nxt.take("pairs", np.complex64, FOLLOW_UP, what), want_more["pairs"], (what, "follow-up pairs"))
            same(nxt.take("points", np.uint8, (256, 256), what), want_more["points"], (what, "follow-up points"))
            same(nxt.take("lines", np.uint8, (256 * lines_m, 256 * lines_m), what), want_more["lines"], (what, "follow-up lines"))
            nxt.free()
        g_in.check((what, "input")), g_more.check((what, "input of the follow-up"))
        g_in.free(), g_more.free(), out.free(), chain.close()


# ---- the zoom -------------------------------------------------------------------------------------------------------

# (fft_size, hop, mode, pair counts): one below, at and above a tile of 128 outputs, which with N = 128 are also N - 1 (no
# row: a zero-byte payload), N and N + 1; N + hop - 1 and N + hop; and rows of 250 bytes on a Bluestein plan
ZOOM_PLANS = [(128, 64, fsea.MODE_MAG_F32, [127, 128, 129, 191, 192]),
              (128, 64, fsea.MODE_DB10_U8, [127, 128, 129, 191, 192]),
              (128, 64, fsea.MODE_COMPLEX_F32, [127, 128, 129, 191, 192]),
              (250, 250, fsea.MODE_DB10_U8, [127, 249, 250, 499, 500])]


@pytest.mark.parametrize("fft_size,hop,mode,pair_counts", ZOOM_PLANS)
@pytest.mark.parametrize("D,L", [(1, 21), (3, 41), (64, fsea.FIR_MAX_TAPS)])
def test_zoom(D, L, fft_size, hop, mode, pair_counts):
    c = lowpass_like_taps(L, 100 * D + L)
    rng = np.random.default_rng(1000 * D + fft_size + mode)
    zooms = [fsea.Zoom(c, D, fft_size, hop, mode) for _ in range(1 + len(INPUT_FILLS))]
    oracle, dtype = zooms[0], fsea._MODE_DTYPE[mode]
    for k, n_out in enumerate(pair_counts):
        n = n_out * D + (D - 1 if k % 4 != 3 else 0)        # n % D != 0 in three cases of four wherever D > 1
        n_rows = (n_out - fft_size) // hop + 1 if n_out >= fft_size else 0
        calls = [n, FOLLOW_UP, D]                            # the follow-ups: 5 samples, then one decimation step
        data = [rng.integers(0, 256, 2 * length, dtype=np.uint8) for length in calls]
        oracle.reset()
        want, pos = [], 0
        for iq in data:
            want.append(oracle.run(iq, CPS, PHASE0, OFFSET + pos, flip=True, pairs=True))
            pos += iq.size // 2
        assert want[0][0].shape == (n_rows, fft_size) and want[0][1].shape == (n_out,)
        for zoom, fill in zip(zooms[1:], INPUT_FILLS):
            zoom.reset()
            pos = 0
            for step, iq in enumerate(data):
                what = (D, L, fft_size, hop, mode, n_out, fill, "call %d" % step)
                m = iq.size // 2
                rows, pairs = zoom.out_rows(m), zoom.out_pairs(m)
                g_in, d_in = fenced(iq, fill)
                out = Outputs(rows=rows * zoom.row_bytes, pairs=8 * pairs)      # no row: the zero-byte payload
                zoom.run_device(d_in, m, out.addr("rows"), CPS, PHASE0, OFFSET + pos, flip=True, d_pairs_ptr=out.addr("pairs"))
                same(out.take("pairs", np.complex64, pairs, what), want[step][1], (what, "pairs"))
                same(out.take("rows", dtype, (rows, fft_size), what), want[step][0], (what, "rows"))
                g_in.check((what, "input"))
                g_in.free(), out.free()
                pos += m
    for z in zooms:
        z.close()


# ---- the filter bank ------------------------------------------------------------------------------------------------

PFB_FRAMES = [0, 1, 2, 127, 128, 129, 257]    # the tile is at most 128 frames and divides neither 129 nor 257


@pytest.mark.parametrize("mode", [fsea.MODE_COMPLEX_F32, fsea.MODE_DB10_U8])
@pytest.mark.parametrize("M,P,q", [(2, 1, 1), (64, 8, 2), (80, 3, 4), (512, 16, 4)])
def test_pfb(M, P, q, mode):
    """Rows, frames and (COMPLEX) the series together; 80 channels are no multiple of the transpose's 32 nor of the frames
    kernel's 64-column chunk.  F = 0 hands in three zero-byte payloads."""
    D = M // q
    complex_mode = mode == fsea.MODE_COMPLEX_F32
    taps = fsea.pfb_prototype(M, P)
    rng = np.random.default_rng(10 * M + P + q + mode)
    pfbs = [fsea.Pfb(taps, M, q, mode) for _ in range(1 + len(INPUT_FILLS))]
    oracle, dtype = pfbs[0], fsea._MODE_DTYPE[mode]
    for F in [f for f in PFB_FRAMES if M < 512 or f <= 129]:
        n = F * D + D - 1                                    # n % D != 0: D - 1 samples stay in the tail
        calls = [n, FOLLOW_UP, D]
        data = [rng.integers(0, 256, 2 * length, dtype=np.uint8) for length in calls]
        oracle.reset()
        want = [oracle.run(iq, flip=True, frames=True, series=complex_mode) for iq in data]
        assert want[0][0].shape == (F, M)
        for pfb, fill in zip(pfbs[1:], INPUT_FILLS):
            pfb.reset()
            for step, iq in enumerate(data):
                what = (M, P, q, mode, F, fill, "call %d" % step)
                m = iq.size // 2
                f = pfb.out_frames(m)
                g_in, d_in = fenced(iq, fill)
                out = Outputs(rows=f * pfb.row_bytes, frames=8 * f * M, series=8 * f * M if complex_mode else 0)
                pfb.run_device(d_in, m, out.addr("rows"), flip=True, d_frames_ptr=out.addr("frames"),
                               d_series_ptr=out.addr("series") if complex_mode else None)
                same(out.take("frames", np.complex64, (f, M), what), want[step][1], (what, "frames"))
                same(out.take("rows", dtype, (f, M), what), want[step][0], (what, "rows"))
                series = out.take("series", np.complex64, (M, f) if complex_mode else (0,), what)
                if complex_mode:
                    same(series, want[step][2], (what, "series"))
                g_in.check((what, "input"))
                g_in.free(), out.free()
    for p in pfbs:
        p.close()


# ---- the audio decoder ----------------------------------------------------------------------------------------------

DEMOD_COUNTS = [1, 49, 105, 2049, 131077]     # 5 MHz -> 48 kHz: out_length 0, 0, 1, 19, 1258


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kind", ["raw", "wbfm"])
def test_demod(kind, K):
    """d_iq is 2-byte aligned: the input stands 2 bytes behind a 16-byte boundary, those 2 bytes filled like the bands.  Two
    calls of n samples, so that both state buffers have been the written one, then the 5-sample follow-up."""
    demods = [fsea.Demod(kind, 5000000, 48000, K) for _ in range(1 + len(INPUT_FILLS))]
    for d in demods:
        for ch in range(K):
            d.set_channel(ch, (50000, -1200000, 0)[ch])
    oracle = demods[0]
    rng = np.random.default_rng(K + len(kind))
    for n in DEMOD_COUNTS:
        data = [rng.integers(0, 256, 2 * length, dtype=np.uint8) for length in (n, n, FOLLOW_UP)]
        oracle.reset()
        want = [oracle.run_u8(iq, flip=True) for iq in data]
        assert want[0].shape == (K, oracle.out_length(n))
        for demod, fill in zip(demods[1:], INPUT_FILLS):
            demod.reset()
            for step, iq in enumerate(data):
                what = (kind, K, n, fill, "call %d" % step)
                m = iq.size // 2
                g_in, d_in = fenced(iq, fill, lead=2)
                assert d_in % 4 == 2
                out = Outputs(audio=8 * K * demod.out_length(m))
                demod.run_device(d_in, m, out.addr("audio"), flip=True)
                same(out.take("audio", np.float64, (K, demod.out_length(m)), what), want[step], what)
                g_in.check((what, "input"))
                g_in.free(), out.free()
    for d in demods:
        d.close()


# ---- the constellation drawers --------------------------------------------------------------------------------------

def draw_inputs():
    """u8, f64 and f32 input, three frames each of an odd number of pairs (frames 1 and 2 of the float inputs start at 8
    and 4 bytes past a 16-byte boundary).  The float frames: the golden's synthetic input (values out of range both ways,
    +-1e30, +-inf, NaN) and endpoints just outside each edge of the image."""
    with np.load(IQ_GOLDEN) as z:
        synthetic = z["in__synthetic"]
    eps = 1.0 / 1024
    edges = np.array([-eps, 0.5, 1.0 + eps, 0.5, 0.5, -eps, 0.5, 1.0 + eps, -eps, -eps, 1.0 + eps, 1.0 + eps, 0.0, 1.0 - eps,
                      1.0 - eps, 0.0, -1e30, 1e30, np.inf, -np.inf, np.nan, 0.25, 0.25, np.nan, 255.999 / 256, -0.999 / 256])
    frame = np.concatenate([synthetic, edges])[:2 * 4107]
    assert frame.size == 2 * 4107
    pairs = frame.reshape(-1, 2)
    f64 = np.stack([pairs, pairs[::-1], np.roll(pairs[:, ::-1], 5, axis=0)]).reshape(3, -1)
    with np.errstate(over="ignore"):
        f32 = f64.astype(np.float32)
    u8 = np.random.default_rng(3).integers(0, 256, (3, 2 * 4107), dtype=np.uint8)
    return {"u8": (fsea.IQ_U8, u8), "f32": (fsea.IQ_F32, f32), "f64": (fsea.IQ_F64, f64)}


@pytest.fixture(scope="module")
def drawing():
    return draw_inputs()


@pytest.mark.parametrize("n_frames", [1, 3, 9])            # 9: a second group of eight frames, seven of them absent
@pytest.mark.parametrize("name", ["u8", "f32", "f64"])
def test_iq_points(drawing, name, n_frames):
    kind, frames = drawing[name]
    frames = np.concatenate([frames] * 3)[:n_frames]
    n = frames.shape[1] // 2
    flip = name == "u8"
    want = np.stack([points_image((frames[f] ^ 0x80) if flip else frames[f].astype(np.float64)) for f in range(n_frames)])
    draw = fsea.IqDraw()
    for fill in INPUT_FILLS:
        what = (name, n_frames, fill)
        g_in, d_in = fenced(frames[:n_frames], fill)
        out = Outputs(image=65536 * n_frames)
        draw.points_device(d_in, kind, n, n_frames, out.addr("image"), flip=flip)
        same(out.take("image", np.uint8, (n_frames, 65536), what), want, what)
        g_in.check((what, "input"))
        g_in.free(), out.free()
    draw.close()


@pytest.mark.parametrize("m", [1, 3, fsea.IQ_MAX_MULTIPLIER])
@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("name", ["u8", "f32", "f64"])
def test_iq_lines(drawing, name, n_frames, m):
    """lines_image up to m = 3; at m = 16 it would cost a 16 Mi-entry bincount per pixel step of the longest segment
    (minutes), so there the oracle is the host form of another object, frame by frame -- the same launch function."""
    kind, frames = drawing[name]
    n = frames.shape[1] // 2
    flip = name == "u8"
    if m <= 3:
        want = np.stack([lines_image((frames[f] ^ 0x80) if flip else frames[f].astype(np.float64), m, n) for f in range(n_frames)])
    else:
        host = fsea.IqDraw()
        want = np.stack([host.lines(frames[f], m=m, flip=flip).ravel() for f in range(n_frames)])
        host.close()
    assert int(want.max()) > 0
    draw = fsea.IqDraw()
    for fill in INPUT_FILLS:
        what = (name, n_frames, m, fill)
        g_in, d_in = fenced(frames[:n_frames], fill)
        out = Outputs(image=(256 * m) ** 2 * n_frames)
        draw.lines_device(d_in, kind, n, n_frames, m, out.addr("image"), flip=flip)
        same(out.take("image", np.uint8, (n_frames, (256 * m) ** 2), what), want, what)
        g_in.check((what, "input"))
        g_in.free(), out.free()
    draw.close()


def test_iq_frames_without_a_point_or_a_segment_are_cleared_and_nothing_else():
    """No pair (points) and a single point (lines) take no kernel: the images are cleared by a memset of their own size."""
    draw = fsea.IqDraw()
    for fill in INPUT_FILLS:
        g_in, d_in = fenced(np.array([10, 20], np.uint8), fill)
        out = Outputs(points=3 * 65536, lines=3 * 768 * 768)
        draw.points_device(d_in, fsea.IQ_U8, 0, 3, out.addr("points"))
        draw.lines_device(d_in, fsea.IQ_U8, 1, 3, 3, out.addr("lines"))
        assert not out.take("points", np.uint8, 3 * 65536, fill).any()
        assert not out.take("lines", np.uint8, 3 * 768 * 768, fill).any()
        g_in.free(), out.free()
    draw.close()


# ---- the persistence picture ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 50, 64, 1040])       # one pixel per lane (1, 50) and sixteen (64, 1040)
def test_persist_image(width):
    """600 rows: 400 of one level per column (counts above SATURATE's 255) and 200 random ones."""
    rng = np.random.default_rng(width)
    rows = np.concatenate([np.tile(rng.integers(0, 256, width, dtype=np.uint8), (400, 1)),
                           rng.integers(0, 256, (200, width), dtype=np.uint8)])
    p = fsea.Persist(width)
    p.add(rows)
    counts = persist_ref.counts_of(rows)
    same(p.counts(), counts, (width, "counts"))
    assert counts.max() >= 400
    for kind in (fsea.PERSIST_MAP_SATURATE, fsea.PERSIST_MAP_LINEAR, fsea.PERSIST_MAP_LOG):
        for full in (0, 150):
            what = (width, kind, full)
            out = Outputs(image=256 * width)
            p.image_device(out.addr("image"), kind, full)
            got = out.take("image", np.uint8, (256, width), what)
            same(got, p.image(kind, full), (what, "host form"))
            same(got, persist_ref.image_of(counts, kind, full or 600), (what, "restatement"))
            out.free()
    p.close()


@pytest.mark.parametrize("n_rows", [1, fsea.PERSIST_RUN_ROWS + 1])
@pytest.mark.parametrize("gap", [0, "16 bytes", "odd"])
@pytest.mark.parametrize("width", [50, 100])               # a partial 16-byte group in the last tile
@pytest.mark.parametrize("name", ["u8", "f32"])
def test_persist_add_reads_the_rows_alone(name, width, gap, n_rows):
    """The input fence of add_device (the counts are the output): rows of `width` elements `pitch` apart in a payload that
    ends with the last row's last element; pitch == width, the next multiple of 16 bytes (the 16-byte kernels wherever a row
    has 16 bytes) and an odd one (element by element).  The gap between two rows is filled like the bands: 0x00 then 0xFF
    for u8, 7.0 (level 255 of the default range) then NaN for f32 -- an element counted from there shows in the counts."""
    esz = 1 if name == "u8" else 4
    per16 = 16 // esz
    pitch = width if gap == 0 else -(-(width + 1) // per16) * per16 if gap == "16 bytes" else width + 1 + (width % 2)
    assert pitch >= width and (gap != "16 bytes" or (pitch * esz) % 16 == 0) and (gap != "odd" or (pitch * esz) % 16)
    rng = np.random.default_rng(width + n_rows)
    if name == "u8":
        rows, gaps = rng.integers(0, 256, (n_rows, width), dtype=np.uint8), (np.uint8(0), np.uint8(0xFF))
    else:
        rows = rng.uniform(-120.0, 20.0, (n_rows, width)).astype(np.float32)
        rows[0, :3] = [np.nan, np.inf, -np.inf]
        gaps = (np.float32(7.0), np.float32(np.nan))
    want = persist_ref.counts_of(rows)
    for fill, gap_value in zip(INPUT_FILLS, gaps):
        what = (name, width, pitch, n_rows, fill)
        laid = np.full(n_rows * pitch, gap_value, rows.dtype)
        laid.reshape(n_rows, pitch)[:, :width] = rows
        laid = laid[:(n_rows - 1) * pitch + width]          # the payload ends with the last row
        g_in, d_in = fenced(laid, fill)
        p = fsea.Persist(width)
        p.add_device(d_in, fsea.PERSIST_U8 if name == "u8" else fsea.PERSIST_F32, n_rows, pitch)
        same(p.counts(), want, what)
        assert p.rows == n_rows
        g_in.check((what, "input"))
        g_in.free(), p.close()


# ---- the detector and the capture -----------------------------------------------------------------------------------

@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("n_blocks", [1, 65, 257])
@pytest.mark.parametrize("block_bytes", [30, 4098, 16386])  # no multiples of 16: under one load, the wave kernel, the slice kernel
def test_detect_sums(block_bytes, n_blocks, flip):
    iq = np.random.default_rng(block_bytes + n_blocks).integers(0, 256, block_bytes * n_blocks, dtype=np.uint8)
    want = numpy_sums(iq, block_bytes, flip)
    det = fsea.Detect()
    for fill in INPUT_FILLS:
        what = (block_bytes, n_blocks, flip, fill)
        g_in, d_in = fenced(iq, fill)
        out = Outputs(sums=24 * n_blocks)
        det.sums_device(d_in, block_bytes, n_blocks, out.addr("sums"), flip=flip)
        same(out.take("sums", np.uint64, (n_blocks, 3), what), want, what)
        g_in.check((what, "input"))
        g_in.free(), out.free()
    det.close()


@pytest.mark.parametrize("m", [1, 3])
def test_capture_burst_lines(m):
    """One burst: three blocks of 48 random bytes, every one above a threshold of 0.  The recording itself stands between
    the two fills for scan_device; the image against the host form and against lines_image on the burst's pairs."""
    bb, n_blocks = 48, 3
    rec = np.random.default_rng(m).integers(0, 256, bb * n_blocks, dtype=np.uint8)
    c = fsea.lowpass_taps(5000000, 200000, 21)
    host = fsea.Capture(c)
    assert host.scan(rec, bb, 0.0) == 1
    n_pairs = host.burst(0).n_pairs
    assert n_pairs == bb * n_blocks // 2
    pairs = host.burst_pairs(0)
    want = host.burst_lines(0, m)
    same(want.ravel(), lines_image(pairs.view(np.float32).astype(np.float64), m, n_pairs), (m, "restatement"))
    assert int(want.max()) > 0
    host.close()
    for fill in INPUT_FILLS:
        what = (m, fill)
        g_in, d_in = fenced(rec, fill)
        cap = fsea.Capture(c)
        assert cap.scan_device(d_in, bb, n_blocks, 0.0) == 1
        same(cap.burst_pairs(0), pairs, (what, "pairs"))
        out = Outputs(image=(256 * m) ** 2)
        cap.burst_lines_device(0, m, n_pairs, out.addr("image"))
        same(out.take("image", np.uint8, (256 * m, 256 * m), what), want, what)
        g_in.check((what, "input"))
        g_in.free(), out.free(), cap.close()


# ---- the trace and the interpolator ---------------------------------------------------------------------------------

def test_trace_frames():
    """One odd geometry (a width that is no multiple of 16, frames that start at every alignment) with a band in front of
    the frames as well as behind them."""
    width, height, m, p, f, s, n = 300, 270, 1, 60, 2, 50, 9
    data = np.random.default_rng(width + s).integers(0, 256, n * s + 3, dtype=np.uint8)
    data[0:4] = [128, 128, 127, 127]
    want, canvas = trace_ref.frames(data, s, n, width, height, m, p, f)
    for fill in INPUT_FILLS:
        what = ("trace", fill)
        tr = fsea.Trace(width, height, m, p, f)
        g_in, d_in = fenced(data, fill)
        out = Outputs(frames=n * width * height)
        tr.frames_device(d_in, data.size, s, n, out.addr("frames"))
        same(out.take("frames", np.uint8, (n, height, width), what), want, what)
        same(tr.canvas(), canvas, (what, "canvas"))
        g_in.check((what, "input"))
        g_in.free(), out.free(), tr.close()


@pytest.mark.parametrize("kind,n", [("u8", 4099), ("f64", 513)])
def test_interp_frames(kind, n):
    """The blocks (push_device) and the weights between the two fills; for f64 those are 0.0 and a NaN."""
    rng = np.random.default_rng(n)
    if kind == "u8":
        a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    else:
        a, b = rng.standard_normal(n), rng.standard_normal(n) * 1e3
    w = np.array([0.0, 0.3, 1.0, 1.0000000000000007, -0.5])
    want = interp_ref.blend_frames(a, b, w)
    for fill in INPUT_FILLS:
        what = (kind, n, fill)
        ip = fsea.Interp(a.dtype, n)
        (g_a, d_a), (g_b, d_b), (g_w, d_w) = fenced(a, fill), fenced(b, fill), fenced(w, fill)
        out = Outputs(frames=want.nbytes)
        ip.push_device(d_a)
        ip.push_device(d_b)
        ip.frames_device(d_w, len(w), out.addr("frames"))
        same(out.take("frames", a.dtype, (len(w), n), what), want, what)
        for g in (g_a, g_b, g_w):
            g.check((what, "input"))
            g.free()
        out.free(), ip.close()


def test_interp_image_frames():
    width, height, iq_size = 37, 23, 10
    rng = np.random.default_rng(7)
    n = 2 * iq_size * iq_size
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    w = np.concatenate([np.linspace(-0.2, 1.2, 6), [np.nan]])
    want = interp_ref.image_frames(a, b, w, width, height, iq_size)
    for fill in INPUT_FILLS:
        what = ("image", fill)
        ip = fsea.Interp(np.uint8, n)
        (g_a, d_a), (g_b, d_b), (g_w, d_w) = fenced(a, fill), fenced(b, fill), fenced(w, fill)
        out = Outputs(images=want.nbytes)
        ip.push_device(d_a)
        ip.push_device(d_b)
        ip.image_frames_device(d_w, len(w), width, height, iq_size, out.addr("images"))
        same(out.take("images", np.uint8, want.shape, what), want, what)
        for g in (g_a, g_b, g_w):
            g.check((what, "input"))
            g.free()
        out.free(), ip.close()


def test_a_zero_byte_payload_is_two_touching_bands():
    g = Guarded(0)
    assert g.addr % 16 == 0 and g.addr == g.buf.ptr.value + GUARD
    g.check("nothing ran")
    assert g.payload(np.uint8, 0).size == 0
    g.free()
