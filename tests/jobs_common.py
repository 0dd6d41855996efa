"""What the GPU tests of the pair stages (tests/test_gpu_measure.py, test_gpu_audio.py, test_gpu_spectra.py) and of their shared
scaffold (tests/test_gpu_jobtable.py) have in common: the Gaussian pairs on their pedestal, the two bit comparisons, the
address of a table, the pedestal of a cut-out and the one call of an object that places float32 outputs."""
import ctypes

import numpy as np

from tests.guarded import FILL, Guarded

OFFSET = 0.5 + 0.5j


def pairs_of(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 1.0, n) + 1j * rng.normal(0.0, 1.0, n) + OFFSET).astype(np.complex64)


def same_float_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_record_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def address(tab):
    return ctypes.addressof(tab) if tab is not None and len(tab) else None


def pedestal(c):
    """0.5 sum(c) over the taps as f32 values, added in order in f64: what a cut-out rests on, as fsea-cutouts computes it"""
    total = 0.0
    for v in np.asarray(c, dtype=np.float64).astype(np.float32).astype(np.float64):
        total += float(v)
    return 0.5 * total


def run_device(obj, d_pairs, n_buffer, table, n_out, count, what, stream=0, wait=None, **settings):
    """one call into a guarded output pre-filled with FILL -> one float32 array per job, count(job) long; no float outside
    the jobs' is written"""
    g = Guarded(4 * n_out)
    obj.run_device(d_pairs.addr, n_buffer, table, g.addr, n_out, stream=stream, **settings)
    if wait is not None:
        wait()
    back = g.payload(np.float32, (n_out,))
    g.check("the %s of %d jobs" % (what, len(table)))
    g.free()
    owned = np.zeros(n_out, bool)
    out = []
    for j in table:
        k = count(j)
        owned[j.out_first:j.out_first + k] = True
        out.append(back[j.out_first:j.out_first + k].copy())
    assert np.all(back[~owned].view(np.uint8) == FILL), "a float that no job owns was written"
    return out
