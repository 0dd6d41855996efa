"""Restatements for the signal capture tests (tests/test_signal_capture_host.py, tests/test_gpu_signal_capture.py): the
reference's detector in exact integer sums and exact rational arithmetic, and the state machine of its signal scene
(lua/signal-detector.lua:89-113) written out literally."""
from fractions import Fraction

import numpy as np

DETECTING, CAPTURING = 1, 2


def sums(block):
    """(sum of the bytes at even offsets, sum of all bytes, sum of their squares) of a uint8 block, as Python ints."""
    b = np.asarray(block, dtype=np.uint8).astype(np.int64)
    return int(b[0::2].sum()), int(b.sum()), int((b * b).sum())


def exact_diffs_total(s, n, mean):
    """sum over the n elements x_i = byte_i / 256 of (x_i - mean)^2, exactly, for the double `mean`."""
    m = Fraction(mean)
    return Fraction(s[2], 65536) - 2 * m * Fraction(s[1], 256) + n * m * m


def scale_about_128(block, divisor):
    """The block with its amplitude divided by `divisor` about 128 (integer division toward minus infinity)."""
    b = np.asarray(block, dtype=np.uint8).astype(np.int64)
    return (128 + (b - 128) // divisor).astype(np.uint8)


def scene(sd, threshold, state=DETECTING):
    """The scene's draw() over the blocks of a recording, one block per call while it detects or captures (the DRAWING
    state consumes no block).  Returns (labels, bursts, state): a label per block -- idle, start, captured, end -- and the
    bursts as lists of block indices; a burst that a previous scan left open (state == CAPTURING) continues as the first
    list, which may then be empty."""
    labels, bursts = [], []
    if state == CAPTURING:
        bursts.append([])
    for i, v in enumerate(sd):
        if state == DETECTING:
            if v > threshold:
                state = CAPTURING
                bursts.append([i])
                labels.append("start")
            else:
                labels.append("idle")
        else:
            if v > threshold:
                bursts[-1].append(i)
                labels.append("captured")
            else:
                state = DETECTING   # DRAWING, then DETECTING again: this block is dropped and starts nothing
                labels.append("end")
    return labels, bursts, state
