"""The ordered-statistic CFAR detector (include/fsea.h: fsea_oscfar_*) restated in numpy, twice, on cfar_ref.levels_of:
detect() by the counting identity over sliding windows and detect_loops(), the definition read out literally (a loop per
row and per cell that collects the clipped training cells, sorts them and takes the r-th) for small shapes.
tests/test_oscfar_host.py holds the two against each other; the GPU tier compares the kernels with detect() bit for bit.
Everything is integer arithmetic in int64."""
import numpy as np

from tests.cfar_ref import levels_of

DEFAULT = (2, 16, 60, 24)


def windows(width, guard, train):
    """Half-open [loL, hiL) and [loR, hiR): the clipped training cells of every column."""
    k = np.arange(width)
    G, T = int(guard), int(train)
    return (np.clip(k - G - T, 0, width), np.clip(k - G, 0, width),
            np.clip(k + G + 1, 0, width), np.clip(k + G + T + 1, 0, width))


def rank_of(n, train, rank):
    """r = (R n + 2T - 1) // 2T = ceil(R n / 2T)"""
    return (int(rank) * n + 2 * int(train) - 1) // (2 * int(train))


def detect(rows, guard=2, train=16, offset=60, rank=24):
    """The mask of a 2-D uint8 or float32 array: uint8, 255 for a hit and 0 otherwise.  By the counting identity: a hit
    exactly when n > 0 and at least r training cells have level + offset < x."""
    x = levels_of(rows)
    n_rows, width = x.shape
    G, T = int(guard), int(train)
    loL, hiL, loR, hiR = windows(width, G, T)
    n = (hiL - loL) + (hiR - loR)
    H = G + T
    beside = np.full((n_rows, width + 2 * H), 1 << 40, np.int64)              # the cells outside the row: below no level
    beside[:, H:H + width] = x + int(offset)
    count = np.zeros((n_rows, width), np.int32)
    for i in range(T):
        for d in (-G - T + i, G + 1 + i):                                      # one training cell of every column at a time
            count += beside[:, H + d:H + d + width] < x
    hit = (n[None, :] > 0) & (count >= rank_of(n, T, rank)[None, :])
    return np.where(hit, 255, 0).astype(np.uint8)


def detect_loops(rows, guard=2, train=16, offset=60, rank=24):
    """The definition literally: for small shapes."""
    x = levels_of(rows)
    n_rows, width = x.shape
    out = np.zeros((n_rows, width), np.uint8)
    for r in range(n_rows):
        for k in range(width):
            cells = [int(x[r, c]) for c in list(range(k - guard - train, k - guard)) + list(range(k + guard + 1, k + guard + train + 1))
                     if 0 <= c <= width - 1]
            n = len(cells)
            if n == 0:
                continue
            z = sorted(cells)[(rank * n + 2 * train - 1) // (2 * train) - 1]   # the r-th smallest, counted from 1
            if int(x[r, k]) > z + offset:
                out[r, k] = 255
    return out
