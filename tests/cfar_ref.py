"""The CFAR spectrum detector (include/fsea.h: fsea_cfar_*) restated in numpy, twice: detect() with prefix sums and
detect_loops(), the definition read out literally (a loop per row, per cell and per training cell) for small shapes.
tests/test_cfar_host.py holds the two against each other; the GPU tier compares the kernels with detect() bit for bit.
Everything is integer arithmetic in int64, so neither form can overflow where the kernels' 32-bit arithmetic does not."""
import math

import numpy as np

U8, F32 = 0, 1
CA, GO, SO = 0, 1, 2
MAX_GUARD, MAX_TRAIN, MAX_OFFSET, F32_SCALE = 64, 256, 1 << 20, 64
LIMIT = 1 << 20
BAND = np.dtype([("first", "<i4"), ("last", "<i4"), ("peak", "<i4"), ("peak_hits", "<u4"), ("hits_sum", "<u8")])


def levels_of_f32(v):
    """t = v * 64 in one rounded f32 multiplication; a NaN and t <= -2^20 give -2^20, t >= 2^20 gives 2^20, otherwise
    rint(t), round half to even."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = v * np.float32(F32_SCALE)
    assert t.dtype == np.float32
    out = np.full(t.shape, -LIMIT, np.int64)
    mid = ~np.isnan(t) & (t > -LIMIT) & (t < LIMIT)
    out[mid] = np.rint(t[mid]).astype(np.int64)
    out[~np.isnan(t) & (t >= LIMIT)] = LIMIT
    return out


def levels_of(rows):
    rows = np.asarray(rows)
    if rows.dtype == np.uint8:
        return rows.astype(np.int64)
    assert rows.dtype == np.float32
    return levels_of_f32(rows)


def _decide(x, nL, SL, nR, SR, offset, method):
    okL = x * nL > SL + offset * nL
    okR = x * nR > SR + offset * nR
    if method == CA:
        return (nL + nR > 0) & (x * (nL + nR) > SL + SR + offset * (nL + nR))
    if method == GO:
        return (nL + nR > 0) & ((nL == 0) | okL) & ((nR == 0) | okR)
    assert method == SO
    return ((nL > 0) & okL) | ((nR > 0) & okR)


def detect(rows, guard=2, train=16, offset=60, method=CA):
    """The mask of a 2-D uint8 or float32 array: uint8, 255 for a hit and 0 otherwise."""
    x = levels_of(rows)
    n, width = x.shape
    G, T = int(guard), int(train)
    prefix = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(x, axis=1)], axis=1)   # prefix[:, c] = sum of cells < c
    k = np.arange(width)
    loL, hiL = np.clip(k - G - T, 0, width), np.clip(k - G, 0, width)                     # half-open [lo, hi)
    loR, hiR = np.clip(k + G + 1, 0, width), np.clip(k + G + T + 1, 0, width)
    nL, nR = hiL - loL, hiR - loR
    SL, SR = prefix[:, hiL] - prefix[:, loL], prefix[:, hiR] - prefix[:, loR]
    hit = _decide(x, nL[None, :], SL, nR[None, :], SR, int(offset), method)
    return np.where(hit, 255, 0).astype(np.uint8)


def detect_loops(rows, guard=2, train=16, offset=60, method=CA):
    """The definition literally: for small shapes."""
    x = levels_of(rows)
    n, width = x.shape
    out = np.zeros((n, width), np.uint8)
    for r in range(n):
        for k in range(width):
            nL = SL = nR = SR = 0
            for c in range(k - guard - train, k - guard):
                if 0 <= c <= width - 1:
                    nL, SL = nL + 1, SL + int(x[r, c])
            for c in range(k + guard + 1, k + guard + train + 1):
                if 0 <= c <= width - 1:
                    nR, SR = nR + 1, SR + int(x[r, c])
            if _decide(int(x[r, k]), np.int64(nL), np.int64(SL), np.int64(nR), np.int64(SR), int(offset), method):
                out[r, k] = 255
    return out


def row_hits_of(mask):
    return (np.asarray(mask) == 255).sum(axis=1).astype(np.uint32)


def hits_of(mask, hits=None):
    """Per-column hit counts, on top of `hits` if given."""
    h = (np.asarray(mask) == 255).sum(axis=0).astype(np.uint32)
    return h if hits is None else (hits + h).astype(np.uint32)


def bands_of(hits, rows, min_fraction, max_gap=0, min_width=1):
    """fsea_cfar_bands restated: a structured array of dtype BAND."""
    hits = np.asarray(hits, dtype=np.uint32)
    found = []
    if rows > 0:
        c_min = max(1, int(math.ceil(min_fraction * float(rows))))
        occupied = [int(k) for k in np.flatnonzero(hits.astype(np.uint64) >= c_min)]
        runs = []
        for k in occupied:
            if runs and k - runs[-1][1] - 1 <= max_gap:
                runs[-1][1] = k
            else:
                runs.append([k, k])
        for first, last in runs:
            if last - first + 1 < min_width:
                continue
            part = hits[first:last + 1]
            peak = first + int(np.argmax(part))                   # argmax: the lowest index of the maximum
            found.append((first, last, peak, int(hits[peak]), int(part.astype(np.uint64).sum())))
    return np.array(found, dtype=BAND)
