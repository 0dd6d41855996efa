"""The time-axis CFAR detector (include/fsea.h: fsea_tcfar_*) restated in numpy, twice.  detect() is the header's one
sentence: the mask of a call is fsea_cfar's mask (tests/cfar_ref.py) of the transposed block of before + n + after rows,
transposed back, rows 0 .. n - 1 of the decided part kept.  detect_loops() reads the definition out literally, a loop per
row, column and training row, for small shapes.  combine() restates the mask operation.  tests/test_tcfar_host.py holds the
two against each other; the GPU tier compares the kernels with detect() bit for bit."""
import numpy as np

from tests import cfar_ref as R

CA, GO, SO = R.CA, R.GO, R.SO
MASK_SET, MASK_OR, MASK_AND = 0, 1, 2


def detect(block, before, n, guard=2, train=16, offset=60, method=CA):
    """block: the rows of a call, context included (2-D uint8 or float32): `before` context rows, then the n decided rows,
    then the context behind them.  Returns the (n, width) uint8 mask of the decided rows."""
    block = np.asarray(block)
    assert block.ndim == 2 and 0 <= before and 0 <= n and before + n <= block.shape[0]
    if block.shape[0] == 0:
        return np.zeros((0, block.shape[1]), np.uint8)
    full = R.detect(np.ascontiguousarray(block.T), guard, train, offset, method).T
    return np.ascontiguousarray(full[before:before + n])


def detect_loops(block, before, n, guard=2, train=16, offset=60, method=CA):
    """The definition literally: rows numbered -before .. rows - before - 1, windows clipped to them."""
    x = R.levels_of(np.asarray(block))
    total, width = x.shape
    out = np.zeros((n, width), np.uint8)
    for r in range(n):
        for k in range(width):
            nL = SL = nR = SR = 0
            for q in range(r - guard - train, r - guard):
                if -before <= q <= total - before - 1:
                    nL, SL = nL + 1, SL + int(x[q + before, k])
            for q in range(r + guard + 1, r + guard + train + 1):
                if -before <= q <= total - before - 1:
                    nR, SR = nR + 1, SR + int(x[q + before, k])
            if R._decide(int(x[r + before, k]), np.int64(nL), np.int64(SL), np.int64(nR), np.int64(SR), int(offset), method):
                out[r, k] = 255
    return out


def combine(old, hit, op):
    """The written mask: `hit` (255 / 0) under MASK_SET; with MASK_OR / MASK_AND joined with `old`, any non-zero byte of
    which counts as set; 255 or 0."""
    old, hit = np.asarray(old) != 0, np.asarray(hit) != 0
    out = hit if op == MASK_SET else (hit | old) if op == MASK_OR else (hit & old)
    assert op in (MASK_SET, MASK_OR, MASK_AND)
    return np.where(out, 255, 0).astype(np.uint8)


def context(total, first, n, reach):
    """(before, after) a call that decides rows first .. first + n - 1 of a recording of `total` rows must be given for cut
    invariance: min(reach, the rows that exist) each side, reach = guard + train."""
    return min(reach, first), min(reach, total - first - n)
