"""The persistence spectrum restated in numpy (include/fsea.h: fsea_persist_*): the level of a u8 or f32 element, the
counts of a set of rows, the three maps of the image, the decay and the traces.  Integer arithmetic throughout, and
np.float32 operations one at a time for the f32 level (a subtraction and a product, each rounded: numpy does not fuse
them), so every comparison against the device is bit for bit."""
import numpy as np

LEVELS = 256
MAP_SATURATE, MAP_LINEAR, MAP_LOG = 0, 1, 2
TRACE_MAX, TRACE_MIN, TRACE_QUANTILE = 0, 1, 2


def scale_of(lo, hi):
    """(float)(256.0 / ((double)hi - (double)lo)) of an f32 range."""
    return np.float32(256.0 / (float(np.float32(hi)) - float(np.float32(lo))))


def levels_of(rows, lo=-100.0, hi=0.0):
    """The level of every element, -1 where an f32 element is not counted (a NaN)."""
    rows = np.asarray(rows)
    if rows.dtype == np.uint8:
        return rows.astype(np.int64)
    assert rows.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = (rows - np.float32(lo)) * scale_of(lo, hi)             # two float32 operations, each rounded
        assert t.dtype == np.float32
        level = np.where(t < 0, 0, np.where(t >= 256, 255, np.trunc(np.where(np.isfinite(t), t, 0)))).astype(np.int64)
    level[np.isnan(t)] = -1
    return level


def counts_of(rows, lo=-100.0, hi=0.0, counts=None):
    """counts[level, column] of a 2-D array of rows, added to `counts` where given."""
    rows = np.asarray(rows)
    width = rows.shape[1]
    out = np.zeros((LEVELS, width), dtype=np.int64) if counts is None else counts.astype(np.int64)
    level = levels_of(rows, lo, hi)
    col = np.broadcast_to(np.arange(width), level.shape)
    ok = level >= 0
    np.add.at(out, (level[ok], col[ok]), 1)
    assert out.max(initial=0) < 1 << 32
    return out.astype(np.uint32)


def log_q(c):
    """q(0) = 0; for c >= 1: e = floor(log2 c), m = ((c << 8) >> e) & 255, q = 256 e + m + 1.  Python integers."""
    c = int(c)
    if c == 0:
        return 0
    e = c.bit_length() - 1
    return 256 * e + (((c << 8) >> e) & 255) + 1


def map_counts(counts, kind, full):
    """The pixel of every count (same shape); full == 0 gives zeros except under SATURATE."""
    c = np.asarray(counts).astype(np.uint64)
    if kind == MAP_SATURATE:
        return np.minimum(c, 255).astype(np.uint8)
    if full == 0:
        return np.zeros(c.shape, np.uint8)
    if kind == MAP_LINEAR:
        return np.minimum(255, c * np.uint64(255) // np.uint64(full)).astype(np.uint8)
    den = max(1, log_q(full) - 1)
    q = np.array([log_q(v) for v in c.ravel()], dtype=np.int64).reshape(c.shape)
    return np.where(c == 0, 0, np.minimum(255, 1 + (q - 1) * 254 // den)).astype(np.uint8)


def image_of(counts, kind, full):
    """image[255 - level, column]: the strongest level is the top row."""
    return map_counts(counts, kind, full)[::-1]


def decay(counts, rows, numerator, denominator):
    c = np.asarray(counts).astype(np.uint64) * np.uint64(numerator) // np.uint64(denominator)
    return c.astype(np.uint32), int(rows) * int(numerator) // int(denominator)


def trace(counts, kind, fraction=0.5):
    counts = np.asarray(counts)
    out = np.zeros(counts.shape[1], np.uint8)
    for k in range(counts.shape[1]):
        col = [int(v) for v in counts[:, k]]
        occupied = [level for level in range(LEVELS) if col[level]]
        if not occupied:
            continue
        if kind == TRACE_MAX:
            out[k] = occupied[-1]
        elif kind == TRACE_MIN:
            out[k] = occupied[0]
        else:
            target = max(1, int(np.ceil(np.float64(fraction) * np.float64(sum(col)))))
            acc = 0
            for level in range(LEVELS):
                acc += col[level]
                if acc >= target:
                    out[k] = level
                    break
    return out
