"""Input families whose spectra have no dominant bin, and those spectra in closed form (numpy, no GPU).

parity.check_float allows every bin 2e-6 of the row's LARGEST bin.  Every other u8 input of the suite -- synth_iq, the
recorded captures, the constant and square-wave frames -- has one or two bins (the offset-binary DC term, a tone) a
hundred to a thousand times above the rest, so that allowance is 1e-3 of an ordinary bin and the L2 norm is the DC
term's: a twiddle a few 1e-5 rad off passes.  The frames made here satisfy a CREST CONDITION on their reference row,

    max |want| <= CREST_MAX * median |want|        over the bins that are compared,

so the unchanged bound speaks for every bin.  It is a condition on the inputs, asserted for every family in
tests/test_flat_host.py, not a measurement of any kernel.

Bytes are written in offset binary (sample = byte / 256, the reference's unpack loop); with flip=True the frames hold the
raw int8 bytes (byte ^ 0x80) that unpack to the same samples.  A frame is a constant background byte `bg` with a few
samples replaced; an impulse's amplitude is what it adds to the background, ((bi - bg) + i (bq - bg)) / 256, and the
transform the kernels compute, X[k] = sum_j (-1)^j w[j] x[j] e^{-2 pi i j k / n}, gives for impulses at p_m

    X[k] = sum_m a_m w[p_m] (-1)^{p_m} e^{-2 pi i p_m k / n}   (+ the background's own spectrum, see below).

Backgrounds: byte 0x00 (sample 0.0: nothing but the impulses), and byte 0x80 (sample 0.5 (1 + i)) for the centred form of
the windowed kernels, which transform w (u - 128) / 256 and add the DC term's spectrum from a table: over a zero
background they would transform -0.5 (1 + i) w and the test would measure the cancellation noise that
build_window_tables documents.  The 0x80 background's spectrum is 0.5 (1 + i) DFT((-1)^j w[j]): for a cosine-sum taper
three to nine bins round n/2 -- and, from the f32 rounding of the weights, a floor in every other bin (Hann: up to 1.1e-7
at 64 points, 1.6e-6 at 2048, 4.8e-6 at 16384, against impulses of 0.06 to 0.56), which the centred form leaves out by
design (build_window_tables: "confined").  That floor is 1e-5 of the impulse, not the 1e-9 a flat comparison needs, so the
reference of such a frame is the oracle's row of the frame MINUS the oracle's row of the bare background
(rows_less_background: the transform is linear, what remains is the oracle's response to the impulses alone, equal to the
closed form within 1e-9 of the impulse) on the bins that lie outside the kernels' table whatever the configuration, and
the oracle's row as it is on those inside it (centred_rings); crest condition and check_float's max over those bins.
The frequency shifter adds 0.5 (1 + i) to every sample after the rotation (src/nrf.c:843-866), a DC term in bin n/2 alone
when there is no taper: shifted rows are compared on every bin but n/2.
"""
from fractions import Fraction
from math import floor

import numpy as np

CREST_MAX = 4.0
BAND = 8
SINGLE = {0x00: (0xff, 0xc0), 0x80: (0xff, 0x40)}    # background byte -> (I, Q) bytes of the single impulse
STRONG = {0x00: (0xfe, 0xc0), 0x80: (0x00, 0x00)}    # the fixed impulse of a pair: exactly twice WEAK's magnitude
WEAK = {0x00: (0x7f, 0x60), 0x80: (0xc0, 0x40)}


def amplitude(pair, bg=0x00):
    return complex(pair[0] - bg, pair[1] - bg) / 256.0


def positions(n):
    """Impulse positions that know nothing of any kernel configuration: n - 1, every d * 2^b < n with d odd <= 31, and 32
    seeded draws; all n positions up to 1024 points.  Every digit value r < 32 at every power-of-two stride s is there as
    the single nonzero digit r * s, so whatever the radix order, every row of every pass table, deferred table and HI / LO
    factor multiplies nonzero data in some frame (tests/test_flat_host.py enumerates radices 2 ... 32)."""
    if n <= 1024:
        return np.arange(n)
    s = {n - 1}
    b = 0
    while (1 << b) < n:
        s.update(d << b for d in range(1, 32, 2) if (d << b) < n)
        b += 1
    s.update(int(p) for p in np.random.default_rng(n).integers(0, n, 32))
    return np.array(sorted(s))


def build_frames(n, placements, bg=0x00, flip=True):
    """(len(placements), 2 n) uint8: frame f is the background with sample p set to bytes (bi, bq) for every
    (p, (bi, bq)) of placements[f]."""
    iq = np.full((len(placements), 2 * n), bg, np.uint8)
    for f, imps in enumerate(placements):
        for p, (bi, bq) in imps:
            iq[f, 2 * p], iq[f, 2 * p + 1] = bi, bq
    return iq ^ np.uint8(0x80) if flip else iq


def spectra(n, placements, bg=0x00, window=None, shift=None, hop=None):
    """The impulses' spectra in closed form, complex128 (len(placements), n); the phase index p k is reduced mod n in
    integers.  `window`: the n weights as the kernel applies them (f32 values).  shift = (cycles_per_sample,
    phase0_cycles): the frequency shifter turns the sample at stream position f * hop + p by that many cycles (bg must be
    0x00: the shifter rotates the offset-binary sample itself).  The background's spectrum and the shifter's DC term are
    not in it."""
    k = np.arange(n, dtype=np.int64)
    hop = n if hop is None else hop
    out = np.zeros((len(placements), n), np.complex128)
    for f, imps in enumerate(placements):
        for p, pair in imps:
            a = amplitude(pair, bg) * (1.0 if window is None else float(window[p])) * (-1.0 if p & 1 else 1.0)
            if shift is not None:
                assert bg == 0x00
                turns = Fraction(shift[1]) + Fraction(shift[0]) * (f * hop + p)      # the doubles as the rationals they are
                a *= np.exp(2j * np.pi * float(turns - floor(turns)))
            out[f] += a * np.exp(-2j * np.pi * ((p * k) % n) / n)
    return out


def impulse_placements(pos, bg=0x00):
    return [[(int(p), SINGLE[bg])] for p in pos]


def pair_placements(pos, bg=0x00, fixed=0):
    """A weak impulse at p beside a fixed one of twice its magnitude at sample `fixed` (p == fixed is left out): a single
    impulse keeps |X| flat under a pure phase error, the interference carries the phase into MAG, dB and pixel rows.
    |X[k]| lies in [|a_s| - |a_w|, |a_s| + |a_w|], a crest of at most 3 (less under a taper with |w[p]| <= |w[fixed]|)."""
    return [[(int(fixed), STRONG[bg]), (int(p), WEAK[bg])] for p in pos if int(p) != int(fixed)]


def impulse_frames(n, flip=True, pos=None, bg=0x00):
    """One impulse per frame at each of `pos` (default positions(n)): every bin has the same size, a crest of 1.
    Returns (bytes, placements)."""
    pl = impulse_placements(positions(n) if pos is None else pos, bg)
    return build_frames(n, pl, bg, flip), pl


def pair_frames(n, flip=True, pos=None, bg=0x00, fixed=0):
    pl = pair_placements(positions(n) if pos is None else pos, bg, fixed)
    return build_frames(n, pl, bg, flip), pl


def crest(want, keep=None):
    a = np.abs(np.asarray(want))
    a = a if keep is None else a[..., keep]
    med = np.median(a, axis=-1)
    return float(np.max(a.max(axis=-1) / med)) if np.all(med > 0) else float("inf")


def sparse_frames(n, nf=8, m=8, seed=0, flip=True):
    """nf frames of m <= 8 impulses at random positions with random bytes over the zero background; a frame whose
    spectrum breaks the crest condition is drawn again.  Returns (bytes, placements)."""
    assert 1 <= m <= 8
    rng = np.random.default_rng([seed, n, m])
    pl = []
    while len(pl) < nf:
        ps = rng.choice(n, size=min(m, n), replace=False)
        imps = [(int(p), (int(rng.integers(1, 256)), int(rng.integers(1, 256)))) for p in ps]
        if crest(spectra(n, [imps])) <= CREST_MAX:
            pl.append(imps)
    return build_frames(n, pl, 0x00, flip), pl


def centred(x):
    """(-1)^j x[j] of interleaved f64 IQ as complex128: the unpack loop of nrf_fft_process' F64 branch."""
    z = np.asarray(x, np.float64).reshape(-1, 2)
    z = z[:, 0] + 1j * z[:, 1]
    z[1::2] *= -1.0
    return z


def noise_f64(n, nf, seed=0):
    """nf frames of zero-mean complex Gaussian noise, sigma 0.2, as interleaved f64 holding f32 values (the kernels take
    f32: the reference then sees the numbers the kernel sees).  A frame that breaks the crest condition is drawn again (the
    largest of n Rayleigh bins is about sqrt(log2 n) medians: 3.7 at 16384 points).  Returns (x of shape (nf, 2 n), f64
    spectra by numpy's FFT, which stands in for no oracle: tests compare with the oracle's or any_size_spectra's)."""
    rng = np.random.default_rng([seed, n])
    xs, ss = [], []
    while len(xs) < nf:
        x = rng.normal(0.0, 0.2, 2 * n).astype(np.float32).astype(np.float64)
        s = np.fft.fft(centred(x))
        if crest(s) <= CREST_MAX:
            xs.append(x)
            ss.append(s)
    return np.stack(xs), np.stack(ss)


def impulses_f64(n, pos, amp=0.75 - 0.5j):
    """f64-input impulse frames: exact zeros and one sample `amp` (f32-exact) at p.  Returns (x (len(pos), 2 n), spectra)."""
    x = np.zeros((len(pos), 2 * n))
    k = np.arange(n, dtype=np.int64)
    s = np.empty((len(pos), n), np.complex128)
    for f, p in enumerate(pos):
        p = int(p)
        x[f, 2 * p], x[f, 2 * p + 1] = amp.real, amp.imag
        s[f] = amp * (-1.0 if p & 1 else 1.0) * np.exp(-2j * np.pi * ((p * k) % n) / n)
    return x, s


def any_size_positions(n):
    """Impulse positions for the sizes without a kernel of their own: all of them up to 32 points; else the last sample,
    eight of the odd-digit-times-power-of-two positions below n (for a four-step size n1 n2 the strides j1 * n2 and the
    small j2 are among them) and 16 seeded odd positions in the upper half of the frame, which have both four-step digits
    nonzero whatever the split (an odd p has j2 != 0, and p >= n / 2 >= n2 has j1 != 0)."""
    if n <= 32:
        return np.arange(n)
    m = 1 << int(n - 1).bit_length()
    base = positions(max(m, 2048))
    base = base[base < n]
    odd = np.minimum(np.random.default_rng(n).integers(n // 2, n, 16) | 1, n - 1 - (n & 1))
    return np.unique(np.r_[base[:: max(1, base.size // 8)][:8], n - 1, odd])


def band_keep(n, half=BAND):
    """The bins farther than `half` from n/2."""
    return np.abs(np.arange(n) - n // 2) > half


def not_dc(n):
    keep = np.ones(n, bool)
    keep[n // 2] = False
    return keep


def rows_less_background(rows_fn, iq, bg_frame):
    """rows_fn(bytes, n_frames) -> the oracle's complex rows; returns the rows of `iq` (frames, 2 n) minus the row of the
    bare background frame: the oracle's response to the impulses alone (module docstring)."""
    iq = np.asarray(iq)
    return rows_fn(iq.ravel(), iq.shape[0]) - rows_fn(np.asarray(bg_frame).ravel(), 1)[0]


def window_positions(n, w, floor=0.1):
    """positions(n) at which the taper leaves at least `floor` of the impulse."""
    pos = positions(n)
    return pos[np.abs(np.asarray(w, np.float64)[pos]) >= floor]


def windowed_case(n, wname, kind, flip=True, pos=None, shift=None):
    """One windowed family: (bytes (frames, 2 n), placements, reference spectra, compared bins or None, f32 weights).
    "hann" takes the 0x80 background, the oracle's rows less the background's and the bins outside the band; "random" the
    zero background and the oracle's rows as they are.  kind "impulse", or "pair" with the fixed impulse where |w| is
    largest.  With shift = (cycles, phase0) the rows are the shifter's (zero background in both forms: the shifter adds
    the 0.5 (1 + i) itself, and its spectrum under the taper is the background that is taken off)."""
    from oracle import oracle as O
    w = taper(wname, n)
    w64 = w.astype(np.float64)
    centred_form = wname != "random"
    assert centred_form or shift is None, "the offset-binary form carries the shifter's DC term through every bin"
    bg = 0x80 if centred_form and shift is None else 0x00
    pos = window_positions(n, w64) if pos is None else np.asarray(pos)[np.abs(w64[np.asarray(pos)]) >= 0.1]
    pl = impulse_placements(pos, bg) if kind == "impulse" else pair_placements(pos, bg, int(np.argmax(np.abs(w64))))
    iq = build_frames(n, pl, bg, flip)
    if shift is None:
        def rows_fn(b, nf):
            return O.rows_windowed(b, nf, n, w64, flip=flip, mode=O.MODE_COMPLEX)
    else:
        def rows_fn(b, nf):
            return O.rows_shifted_windowed(b, nf, n, shift[0], w64, shift[1], flip=flip, mode=O.MODE_COMPLEX)
    full = rows_fn(iq.ravel(), len(pl))
    if not centred_form:
        return iq, pl, full, None, w
    inner, outer = centred_rings(n)
    want = np.where(inner, full, full - rows_fn(build_frames(n, [[]], bg, flip).ravel(), 1)[0])
    return iq, pl, want, inner | outer, w


def centred_rings(n):
    """The bins on which a centred-form row is compared, as two masks.  The kernels add the DC term's spectrum from a
    table of the bins [n/2 - n/RL, n/2 + n/RL), RL the last radix of the size's configuration, whatever that is: between
    4 and 32.  Inner ring, BAND < |k - n/2| < n/32: inside every such table, the row holds the background's floor and
    the reference is the oracle's row as it is.  Outer ring, |k - n/2| > n/4: outside every such table, the floor is left
    out and the reference is the oracle's row less the background's.  The bins between belong to one or the other by
    configuration and are not compared."""
    d = np.abs(np.arange(n) - n // 2)
    return (d > BAND) & (d < n // 32), d > n // 4


def half_overlap_stream(n, nf, mode_pairs=True):
    """A u8 stream (raw int8 bytes, flip=True) for nf frames at hop n/2 in which every frame is a pair frame: blocks of n/2
    samples, the strong impulse at sample 0 of every even block, a weak one at a position of its own in every odd block.
    Frame 2 j holds (0, n/2 + o_j), frame 2 j + 1 holds (o_j, n/2): consecutive frames share half a frame and no frame
    holds two strong impulses.  Returns (bytes, placements per frame)."""
    h = n // 2
    n_blocks = nf + 1
    offs = positions(n)
    offs = offs[(offs > 0) & (offs < h)]
    stream = np.zeros(2 * n_blocks * h, np.uint8)
    per_block = []
    for b in range(n_blocks):
        if b % 2 == 0:
            per_block.append((0, STRONG[0x00]))
        else:
            per_block.append((int(offs[(b // 2 * 7) % offs.size]), WEAK[0x00]))
        p, (bi, bq) = per_block[-1]
        stream[2 * (b * h + p)], stream[2 * (b * h + p) + 1] = bi, bq
    pl = [[per_block[f], (per_block[f + 1][0] + h, per_block[f + 1][1])] for f in range(nf)]
    return stream ^ np.uint8(0x80), pl


def turn_residue_class(want, radians=2e-5, residue=3, modulus=8):
    """A reference row with the bins of one residue class turned by `radians`: what a twiddle-table entry that far off does
    to the bins it feeds.  For the tests of the comparison's own teeth."""
    out = np.array(want, np.complex128)
    out[..., residue::modulus] *= np.exp(1j * radians)
    return out


def check_rows(check, got, want, what, labels, keep=None, per="bin"):
    """check(got[f], want[f]) frame by frame (one call per frame: the bound's max is that frame's), on the bins `keep`;
    a failure names `what`, the frame's label (its impulse positions) and the worst bin.  Returns the worst per-bin
    relative error over all frames, |got - want| / |want| (per="median": over the frame's median |want|, for noise
    frames, whose smallest bins are as small as one likes): a figure to record, no bound."""
    worst = 0.0
    for f in range(len(want)):
        g = np.asarray(got[f])
        w = np.asarray(want[f])
        if keep is not None:
            g, w = g[keep], w[keep]
        err = np.abs(g.astype(np.complex128 if np.iscomplexobj(w) else np.float64) - w)
        k = int(np.argmax(err))
        try:
            check(g, w)
        except AssertionError as e:
            bins = np.arange(len(want[f])) if keep is None else np.flatnonzero(keep)
            raise AssertionError("%s, frame %d (%s): %s; worst bin %d: got %r, want %r" % (
                what, f, labels[f], str(e).splitlines()[0], int(bins[k]), g[k], w[k])) from None
        nz = np.abs(w) > 0
        if per == "median":
            worst = max(worst, float(err.max() / np.median(np.abs(w))))
        elif nz.any():
            worst = max(worst, float(np.max(err[nz] / np.abs(w[nz]))))
    return worst


def label(imps):
    return "impulses at " + ", ".join(str(p) for p, _ in imps)


def labels(placements):
    return [label(imps) for imps in placements]


def check_mode_rows(got, spec, mode, what, names, keep=None, per="bin"):
    """Rows of plan mode `mode` against f64 spectra, frame by frame through tests/parity.py as it stands: check_float for
    modes 0, 3, 4 (the oracle's magnitude loop; plain |X| where bins are left out, the patched bin n/2 among them),
    check_u8 for the pixel modes, check_db_bins for mode 5.  Returns check_rows' figure (mode 5: the worst excess over the
    allowance carried through the logarithm, in dB; pixels: the number of pixels one grey level off)."""
    from tests import parity
    if mode in (0, 3, 4):
        want = spec if mode == 3 else (np.abs(spec) if keep is not None else parity.rows_of_spectra(spec, mode))
        return check_rows(parity.check_float, got, want, what, names, keep, per)
    assert keep is None
    figure = -np.inf if mode == 5 else 0
    for f in range(len(spec)):
        try:
            if mode == 5:
                figure = max(figure, parity.check_db_bins(got[f], parity.rows_of_spectra(spec[f:f + 1], 5)[0], np.abs(spec[f])))
            else:
                figure += parity.check_u8(got[f], parity.rows_of_spectra(spec[f:f + 1], mode)[0])
        except AssertionError as e:
            raise AssertionError("%s, mode %d, frame %d (%s): %s" % (what, mode, f, names[f], str(e).splitlines()[0])) from None
    return figure


def taper(name, n):
    """The two tapers of the windowed tests as f32 weights: "hann" (cosine sum: the kernels' centred form) and "random"
    (uniform in [-1, 2): the offset-binary form)."""
    if name == "random":
        return np.random.default_rng(n).uniform(-1.0, 2.0, n).astype(np.float32)
    from oracle import oracle as O
    return O.window(name, n).astype(np.float32)
