"""The polyphase filter bank of include/fsea.h (fsea_pfb_*) restated in f64 numpy, twice: pfb_direct, the definition channel
by channel -- mix to zero with a phase tied to the stream position, filter by the prototype, keep every D-th output -- and
pfb_frames_reference, the polyphase sums with the rotated store that the kernel computes, whose rows (rows_of: the plan's
(-1)^m centring and a DFT) equal the direct form because M is even.  tile_shape restates the kernel's tile rule so that the
GPU tests can put call lengths on its seams."""
import numpy as np


def u8_to_complex(iq, flip):
    b = np.asarray(iq, dtype=np.uint8)
    b = b ^ 0x80 if flip else b
    return b[0::2] / 256.0 + 1j * (b[1::2] / 256.0)


def _extend(u8, flip, L, tail):
    x = u8_to_complex(u8, flip)
    tail = np.zeros(L - 1, dtype=np.complex128) if tail is None else np.asarray(tail, dtype=np.complex128)
    assert tail.size == L - 1
    x_ext = np.concatenate([tail, x])
    return x, x_ext, x_ext[x_ext.size - (L - 1):]


def pfb_direct(u8, flip, taps, M, D, tail=None, s0=0, columns=None):
    """X_t[k] = sum_{j < L} c[j] x_ext[t D + j] e^{-2 pi i (k - M/2)(s0 + t D + j) / M}, t < n // D, one channel k at a time
    (all of them, or `columns`).  Returns (rows of shape (F, len(columns)), the next tail)."""
    c = np.asarray(taps, dtype=np.float64)
    L = c.size
    x, x_ext, next_tail = _extend(u8, flip, L, tail)
    F = x.size // D
    columns = np.arange(M) if columns is None else np.asarray(columns)
    rows = np.zeros((F, columns.size), dtype=np.complex128)
    if F == 0:
        return rows, next_tail
    step = x_ext.strides[0]
    windows = np.lib.stride_tricks.as_strided(x_ext, (F, L), (D * step, step)) * c     # c[j] x_ext[t D + j]
    pos = (s0 + D * np.arange(F, dtype=np.int64)[:, None] + np.arange(L, dtype=np.int64)[None, :]) % M   # s0 + t D + j
    unit = np.exp(-2j * np.pi * np.arange(M) / M)
    for i, k in enumerate(columns):
        rows[:, i] = (windows * unit[((int(k) - M // 2) * pos) % M]).sum(axis=1)          # channel k mixed to zero, filtered
    return rows, next_tail


def pfb_frames_reference(u8, flip, taps, M, D, tail=None, s0=0, variant=""):
    """v_t[r] = sum_p c[p M + r] x_ext[t D + p M + r], frames[t][(r + s0 + t D) mod M] = v_t[r].  Returns (frames of shape
    (F, M), the next tail).  `variant` breaks it on purpose (the tests' teeth): "no_rotation", "no_s0" (rotation by t D
    alone), "branch_major" (taps read as c[r P + p])."""
    c = np.asarray(taps, dtype=np.float64)
    L = c.size
    P = L // M
    assert P * M == L
    x, x_ext, next_tail = _extend(u8, flip, L, tail)
    F = x.size // D
    frames = np.zeros((F, M), dtype=np.complex128)
    cb = c.reshape(M, P).T if variant == "branch_major" else c.reshape(P, M)
    for t in range(F):
        v = (cb * x_ext[t * D:t * D + L].reshape(P, M)).sum(axis=0)
        shift = {"no_rotation": 0, "no_s0": t * D}.get(variant, s0 + t * D) % M
        frames[t] = np.roll(v, shift)
    return frames, next_tail


def rows_of(frames):
    """The plan's COMPLEX rows of f32-pair frames: (-1)^m centring, then the DFT."""
    M = frames.shape[-1]
    return np.fft.fft(frames * (1.0 - 2.0 * (np.arange(M) % 2)), axis=-1)


def tile_shape(M, P, q):
    """(C, T): the columns and frames of a workgroup's tile, the rule of pfb_shape in frequensea_amd/csrc/fsea_pfb.hip and
    include/fsea.h -- the smallest LDS image (2560, 5120, 10240 samples) and in it the widest C of min(M, 256), 128, 64 that
    leave T >= twice the extra rows; 64 columns in the largest image where none does."""
    extra = (2 * ((P + 1) // 2) - 1) * q

    def tile(cap, width):
        C = min(M, width)
        slots = 256 // C
        T = min(cap // C - extra, 128)
        return C, T - T % slots if T >= slots else T

    for cap in (2560, 5120, 10240):
        for width in (256, 128, 64):
            C, T = tile(cap, width)
            if T >= 1 and T >= 2 * extra:
                return C, T
    return tile(10240, 64)


def branch_normalised_taps(M, P, seed):
    """Positive random taps with every branch summing to 1: S = sum_p |c[p M + r]| = 1 and a DC gain of 1 per branch, the
    premises (S < 2, outputs of the size of the input) of tests/test_gpu_fir.py's bounds."""
    c = np.abs(np.random.default_rng(seed).standard_normal((P, M))) + 1e-3
    return (c / c.sum(axis=0)).ravel()


def tone_bytes(M, frames, offset_channels=10.5, amp=100.0, sigma=1.0, seed=1):
    """Raw int8 IQ bytes: a tone of amplitude `amp` at offset_channels channels of M above the centre plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    n = M * frames
    s = amp * np.exp(2j * np.pi * offset_channels / M * np.arange(n))
    iq = np.empty(2 * n)
    iq[0::2] = s.real + rng.normal(0, sigma, n)
    iq[1::2] = s.imag + rng.normal(0, sigma, n)
    return np.clip(np.rint(iq), -128, 127).astype(np.int8).view(np.uint8)


def leakage(mean_rows, M=128):
    """(the two largest columns, the worst column at least 3 away from both and more than 1 from M / 2, over the peak)."""
    top = np.argsort(mean_rows)[-2:]
    k = np.arange(M)
    far = (np.abs(k - top[0]) >= 3) & (np.abs(k - top[1]) >= 3) & (np.abs(k - M // 2) > 1)
    return set(int(v) for v in top), float(mean_rows[far].max() / mean_rows.max())
