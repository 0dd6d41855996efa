"""Shared parity checks: a candidate (HIP kernel on the GPU, or the same kernel source run
through tests/emu on the CPU) against the f64 oracle.

Stated tolerance (fp32 transform vs f64 reference, BASELINE.json "within a stated float
tolerance"):
  float rows : ||got - want||_2 / ||want||_2 <= 1e-6, and per bin
               |got - want| <= 2e-6 * max(want) (+1e-6 absolute floor)
  complex    : the same on the complex values
  dB (f32)   : compared through power, see check_db
  u8 pixels  : exact on >= 99.9 % of pixels, |diff| <= 1 elsewhere (the reference truncates
               a double; a 1-ulp log difference can move a value across an integer boundary)
"""
import numpy as np

from oracle import oracle as O

ORACLE_MODE = {0: O.MODE_MAG, 1: O.MODE_DB10_U8, 2: O.MODE_DB5_U8_DCFIX, 3: O.MODE_COMPLEX,
               4: O.MODE_MAG_NODC, 5: O.MODE_DB_F64}

REL_L2_TOL = 1e-6
PER_BIN_TOL = 2e-6


def check_float(got, want):
    got = np.asarray(got, dtype=np.complex128 if np.iscomplexobj(got) else np.float64)
    scale = float(np.max(np.abs(want))) if want.size else 1.0
    den = float(np.linalg.norm(want))
    rel = float(np.linalg.norm(got - want)) / den if den > 0 else float(np.linalg.norm(got - want))
    worst = float(np.max(np.abs(got - want))) if want.size else 0.0
    assert rel <= REL_L2_TOL, "relative L2 error %.3e > %.1e" % (rel, REL_L2_TOL)
    assert worst <= PER_BIN_TOL * scale + 1e-6, "per-bin error %.3e > %.3e" % (worst, PER_BIN_TOL * scale + 1e-6)
    return rel, worst


def check_u8(got, want):
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max(initial=0) <= 1, "pixel differs by %d" % diff.max()
    bad = np.count_nonzero(diff)
    assert bad <= max(1, int(1e-3 * want.size)), "%d of %d pixels differ" % (bad, want.size)
    return bad


def check_db(got, want_db, want_mag_nodc):
    """10*log10(p + 1e-20) in f32: compare where the bin is not numerically empty."""
    floor = 1e-5 * float(np.max(want_mag_nodc))
    keep = want_mag_nodc > floor
    err = np.abs(np.asarray(got, dtype=np.float64) - want_db)[keep]
    # d(dB) = 8.69 * d(mag)/mag ; mags above the floor are accurate to ~2e-6*max/floor relative
    assert err.max(initial=0.0) <= 8.69 * PER_BIN_TOL / 1e-5 + 1e-3


def check_db_bins(got, want_db, want_mag_nodc):
    """dB rows (mode 5) bin by bin, for rows without numerically empty bins (tests/flat_ref.py).  check_db allows 1.7 dB
    because it is written for rows with a dynamic range of 1e5; here every bin gets check_float's per-bin allowance on its
    magnitude, 2e-6 * max + 1e-6, carried through the logarithm, plus the logarithm's own error L:
        |got - want| <= 20 log10(1 + (2e-6 * max + 1e-6) / mag[k]) + L[k].
    L: the kernels form (10 log10 2) * v_log_f32(p + 1e-20).  v_log_f32 (base 2) is stated as "1ULP accuracy, denormals are
    flushed" in AMD's "Graphics Core Next Architecture, Generation 3" ISA reference (chapter 13, VOP1 opcodes, V_LOG_F32;
    the later ISA guides list the opcode without a figure): 2^-23 of |log2 p|.  The product with the f32 constant adds one
    rounding and the constant's own, 2^-24 each: together 2^-22 of |dB|.  Near p = 1 the result vanishes and nothing
    promises an error relative to it, so the level is taken as at least one octave (3.01 dB).  p = re^2 + im^2 + 1e-20
    carries three f32 roundings (one under contraction), 3 * 2^-24 relative, 10 log10(e) times that in dB.
    Returns the worst excess over the first term alone, in dB (negative: inside it without L): what L has to cover."""
    want_db = np.asarray(want_db, dtype=np.float64)
    mag = np.asarray(want_mag_nodc, dtype=np.float64)
    assert mag.min(initial=1.0) > 0.0, "check_db_bins is for rows without empty bins"
    err = np.abs(np.asarray(got, dtype=np.float64) - want_db)
    through_log = 20.0 * np.log10(1.0 + (PER_BIN_TOL * float(np.max(mag)) + 1e-6) / mag)
    octave = 10.0 * 0.30102999566398120
    bound = through_log + 2.0 ** -22 * np.maximum(np.abs(want_db), octave) + 10.0 * np.log10(np.e) * 3.0 * 2.0 ** -24
    k = int(np.argmax(err - bound))
    assert np.all(err <= bound), "dB error %.3e > %.3e at bin %d" % (err.flat[k], bound.flat[k], k)
    return float(np.max(err - through_log))


def check_mode(got, iq, n, n_frames, hop, flip, mode):
    want = O.rows(iq, n_frames, n, hop=hop, flip=flip, mode=ORACLE_MODE[mode])
    if mode in (1, 2):
        return check_u8(got, want)
    if mode == 5:
        return check_db(got, want, O.rows(iq, n_frames, n, hop=hop, flip=flip, mode=O.MODE_MAG_NODC))
    return check_float(got, want)


def any_size_spectra(iq, n, nf, hop, flip, exact=None):
    """f64 spectra of nf frames for a transform size the oracle's power-of-two FFT does not take: the oracle's own unpack
    loop in front of its O(n^2) long-double DFT (`exact`, by default for n <= 1001) or of numpy's f64 FFT (an O(n^2)
    check of a large n would take minutes)."""
    exact = n <= 1001 if exact is None else exact
    iq = np.ascontiguousarray(iq, dtype=np.uint8).ravel()
    spectra = np.empty((nf, n), dtype=np.complex128)
    for f in range(nf):
        raw = iq[2 * f * hop: 2 * (f * hop + n)]
        x = O.unpack_center_u8(O.flip_u8(raw) if flip else raw)
        spectra[f] = O.dft_naive(x) if exact else np.fft.fft(x)
    return spectra


def rows_of_spectra(spectra, mode):
    """The oracle's magnitude / pixel loops over f64 spectra (modes 4 and 5, for which it exports no row function: the
    expressions of its orc_epilogue)."""
    if mode == 0:
        return np.stack([O.mag_row(s) for s in spectra])
    if mode in (1, 2):
        return np.stack([O.db_u8_row(s, 10.0 if mode == 1 else 5.0, int(mode == 2)) for s in spectra])
    if mode == 3:
        return spectra
    if mode == 4:
        return np.abs(spectra)
    return 10.0 * np.log10(spectra.real ** 2 + spectra.imag ** 2 + 1.0e-20)


def check_spectra(got, spectra, mode):
    """check_mode against f64 spectra that the caller computed (and may share between modes)."""
    want = rows_of_spectra(spectra, mode)
    if mode in (1, 2):
        return check_u8(got, want)
    if mode == 5:
        return check_db(got, want, np.abs(spectra))
    return check_float(got, want)


def check_any_size(got, iq, n, nf, hop, flip, mode, exact=None):
    """check_mode for the sizes without a kernel of their own (Bluestein, four-step): same bounds, reference any_size_spectra."""
    return check_spectra(got, any_size_spectra(iq, n, nf, hop, flip, exact), mode)


def check_mode_shifted(got, iq, n, n_frames, hop, flip, mode, cycles_per_sample, phase0_cycles=0.0):
    """check_mode for the frequency-shifted path (oracle: orc_rows_shifted)."""
    kw = dict(hop=hop, flip=flip)
    want = O.rows_shifted(iq, n_frames, n, cycles_per_sample, phase0_cycles, mode=ORACLE_MODE[mode], **kw)
    if mode in (1, 2):
        return check_u8(got, want)
    if mode == 5:
        return check_db(got, want, O.rows_shifted(iq, n_frames, n, cycles_per_sample, phase0_cycles,
                                                  mode=O.MODE_MAG_NODC, **kw))
    return check_float(got, want)


def check_mode_windowed(got, iq, n, n_frames, hop, flip, mode, window):
    """check_mode for a plan with a taper window (oracle: orc_rows_windowed, x[j] = (-1)^j w[j] u8[j] / 256)."""
    w = np.asarray(window, dtype=np.float32).astype(np.float64)   # the weights the kernel applies are the f32 values
    kw = dict(hop=hop, flip=flip)
    want = O.rows_windowed(iq, n_frames, n, w, mode=ORACLE_MODE[mode], **kw)
    if mode in (1, 2):
        return check_u8(got, want)
    if mode == 5:
        return check_db(got, want, O.rows_windowed(iq, n_frames, n, w, mode=O.MODE_MAG_NODC, **kw))
    return check_float(got, want)
