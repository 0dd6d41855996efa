"""GPU tier: the life cycle of the device objects and plans behind fsea.py's wrappers -- create, use, reset, destroy.
Every struct behind them releases its HIP resources through members that release themselves (csrc/fsea_internal.h), so what
is checked here is what a forgotten or misordered member would break: a cycle repeated 32 times gives the same bits, a reset
object equals a fresh one, the capture's pairs survive the move of their buffer, the demodulator's index tables survive
their moves inside the cache, and device memory comes back.

Everything is compared bit for bit: the same kernels on the same input, whatever object runs them."""
import torch  # torch's HIP runtime first, then the library (loaded globally), as scripts/demod_rate.py does

import numpy as np
import pytest

from frequensea_amd import fsea

pytestmark = pytest.mark.gpu

CYCLES = 32


def taps():
    return fsea.lowpass_taps(5000000, 200000, 21)


def data(seed, n_bytes):
    return np.random.default_rng(seed).integers(0, 256, n_bytes, dtype=np.uint8)


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- one small call per kind of object: (create, call on `seed`'s data); the smallest shapes at which each path still runs

FIR_BYTES = 2 * (4096 + 3)        # two tiles and an edge
ZOOM_BYTES = 2 * 4 * 256          # D = 4: 256 decimated pairs, two rows of 128
PFB_BYTES = 2 * (32 * 40 + 5)     # M = 64 at oversampling 2, a frame every 32 samples: 40 frames and an edge
DEMOD_SAMPLES = 1 << 14
INTERP_N = 4096
WEIGHTS = [0.0, 0.3, 1.0]
BLOCK = 4096                      # capture and detect: eight blocks


def make_fir():
    return fsea.Fir(taps())


def call_fir(f, seed):
    return f.run_u8(data(seed, FIR_BYTES))


def make_chain():
    return fsea.Chain(taps())


def call_chain(c, seed):
    r = c.run(data(seed, FIR_BYTES), points=True, lines_m=1, pairs=True)
    return r["pairs"], r["points"], r["lines"]


def make_zoom():
    return fsea.Zoom(taps(), 4, 128)


def call_zoom(z, seed):
    return z.run(data(seed, ZOOM_BYTES), 0.0123, pairs=True)


def make_pfb():
    return fsea.Pfb(fsea.pfb_prototype(64, 16), 64, 2, fsea.MODE_COMPLEX_F32)   # L = 1024: a tail above FSEA_FIR_MAX_TAPS


def call_pfb(b, seed):
    return b.run(data(seed, PFB_BYTES), frames=True, series=True)


def make_demod():
    d = fsea.Demod("wbfm", 10000000, 48000, n_channels=2)
    d.set_channel(0, 250000)
    d.set_channel(1, -1200000)         # phases as a reset leaves them: (1, 0)
    return d


def call_demod(d, seed, n=DEMOD_SAMPLES):
    return d.run_u8(data(seed, 2 * n))


def make_interp():
    return fsea.Interp(np.uint8, INTERP_N)


def call_interp(p, seed):
    p.push(data(seed, INTERP_N))
    p.push(data(seed + 1000, INTERP_N))
    return p.frames(WEIGHTS)


def make_trace():
    return fsea.Trace(256, 256, m=1, pixel_inc=40, fade=3)


def call_trace(t, seed):
    return t.frames(data(seed, 3 * 64), 64, 3)


def make_iq_draw():
    return fsea.IqDraw()


def call_iq_draw(d, seed):
    iq = data(seed, 2 * 4096)
    return d.points(iq), d.lines(iq, 1)


def make_detect():
    return fsea.Detect()


def recording(seed, pattern):
    """Blocks of BLOCK bytes: L loud (uniform bytes, sd about 74), q quiet (127 .. 129, sd below 1)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 256, BLOCK, dtype=np.uint8) if c == "L" else rng.integers(127, 130, BLOCK, dtype=np.uint8)
                           for c in pattern])


THRESHOLD = 20.0


def call_detect(d, seed):
    return d.run(recording(seed, "qLLqLqqL"), BLOCK)


def make_capture():
    return fsea.Capture(taps())


def call_capture(c, seed):
    n = c.scan(recording(seed, "qLLqLqqL"), BLOCK, THRESHOLD)
    assert n == 3
    return [c.burst_pairs(k) for k in range(n)] + [c.burst_lines(0, 1)]


def make_plan_window():
    p = fsea.Plan(128)
    p.set_window("hann")
    return p


def make_plan_bluestein():
    return fsea.Plan(100)


def make_plan_fourstep():
    return fsea.Plan(1 << 15)


def call_plan(p, seed):
    return p.exec_host(data(seed, 2 * p.fft_size * 3), 3)


OBJECTS = {
    "fir": (make_fir, call_fir),
    "zoom": (make_zoom, call_zoom),
    "pfb": (make_pfb, call_pfb),
    "demod": (make_demod, call_demod),
    "interp": (make_interp, call_interp),
    "trace": (make_trace, call_trace),
    "iq_draw": (make_iq_draw, call_iq_draw),
    "chain": (make_chain, call_chain),
    "detect": (make_detect, call_detect),
    "capture": (make_capture, call_capture),
    "plan_window": (make_plan_window, call_plan),
    "plan_bluestein": (make_plan_bluestein, call_plan),
    "plan_fourstep": (make_plan_fourstep, call_plan),
}


@pytest.mark.parametrize("kind", sorted(OBJECTS))
def test_create_use_destroy_cycles_give_the_same_bits(kind):
    make, call = OBJECTS[kind]
    first = None
    for cycle in range(CYCLES):
        obj = make()
        got = call(obj, 7)
        obj.close()
        if first is None:
            first = got
            assert all(np.asarray(x).size for x in (got if isinstance(got, (tuple, list)) else [got])), "an empty output checks nothing"
        assert same(got, first), (kind, cycle)


@pytest.mark.parametrize("kind", ["fir", "zoom", "pfb", "chain", "demod", "interp", "trace"])
def test_reset_equals_a_fresh_object(kind):
    make, call = OBJECTS[kind]
    used, fresh = make(), make()
    a = call(used, 1)
    used.reset()
    after_reset, want = call(used, 2), call(fresh, 2)
    assert same(after_reset, want), kind
    assert not same(a, want), "data A and data B must differ for the comparison to mean anything"
    used.close()
    fresh.close()


def test_a_failed_zoom_create_leaves_nothing_half_made():
    """Mode 99 fails in the inner plan's create: inside the initialiser, after the object and its staging stream exist.  The
    status is the plan's own, and a valid zoom created right after it works."""
    with pytest.raises(fsea.FseaError) as zoom_error:
        fsea.Zoom(taps(), 4, 128, mode=99)
    with pytest.raises(fsea.FseaError) as plan_error:
        fsea.Plan(128, mode=99)
    assert str(zoom_error.value) == str(plan_error.value)
    z, ref = make_zoom(), make_zoom()
    assert same(call_zoom(z, 3), call_zoom(ref, 3))
    z.close()
    ref.close()


def test_a_failed_chain_create_leaves_nothing_half_made():
    """A device index one past the last fails in the shared create sequence, after the taps are found good: the text is the
    filter's for the same index, and a valid chain created right after it works."""
    no_device = fsea.device_count()
    with pytest.raises(fsea.FseaError) as chain_error:
        fsea.Chain(taps(), device=no_device)
    with pytest.raises(fsea.FseaError) as fir_error:
        fsea.Fir(taps(), device=no_device)
    assert str(chain_error.value) == str(fir_error.value)
    c, ref = make_chain(), make_chain()
    assert same(call_chain(c, 3), call_chain(ref, 3))
    c.close()
    ref.close()


def test_the_captures_pairs_survive_a_growth():
    """Blocks of 4096 bytes are 2048 pairs.  Scan 1 has one loud block: the buffer holds 2048 + 512 + 512 pairs.  Scan 2 has
    four loud blocks in two new bursts and needs 10240, so the buffer moves: burst 0's pairs are the same bits at a new
    address, and every burst is what one fsea.Chain gives on the same blocks in the same order."""
    first, second = recording(11, "qqLqqqqq"), recording(12, "qLLqLLqq")
    cap, chain = make_capture(), make_chain()
    assert cap.scan(first, BLOCK, THRESHOLD) == 1
    info = cap.burst(0)
    assert (info.first_block, info.n_blocks, info.n_pairs, info.open) == (2, 1, 2048, 0)
    before, address = cap.burst_pairs(0), info.d_pairs
    assert cap.scan(second, BLOCK, THRESHOLD) == 3
    assert cap.burst(0).d_pairs != address, "the buffer did not move: the scan checks no growth"
    assert same(cap.burst_pairs(0), before)
    blocks = lambda rec, lo, hi: rec[lo * BLOCK:hi * BLOCK]
    want = [chain.run(b, pairs=True)["pairs"] for b in (blocks(first, 2, 3), blocks(second, 1, 3), blocks(second, 4, 6))]
    assert [(cap.burst(k).first_block, cap.burst(k).n_blocks) for k in range(3)] == [(2, 1), (9, 2), (12, 2)]
    for k in range(3):
        assert same(cap.burst_pairs(k), want[k]), k
    cap.close()
    chain.close()


def test_demod_evicts_moved_index_tables_correctly():
    """Ten distinct lengths on one object whose cache holds eight tables: the ninth and tenth each evict the least recently
    used one and the tables behind it move down.  Then the first length again (evicted by now).  A second object given
    the same inputs in calls of the same lengths returns the same audio, bit for bit."""
    lengths = [DEMOD_SAMPLES + 16 * k for k in range(10)] + [DEMOD_SAMPLES]
    one, two = make_demod(), make_demod()
    got = [call_demod(one, 20 + i, n) for i, n in enumerate(lengths)]
    want = [call_demod(two, 20 + i, n) for i, n in enumerate(lengths)]
    assert all(g.size for g in got)
    for i in range(len(lengths)):
        assert same(got[i], want[i]), (i, lengths[i])
    one.close()
    two.close()


MIB = 1 << 20


def cycle_interp():
    p = fsea.Interp(np.uint8, 1 << 22)          # two blocks of 4 MiB
    p.frames([0.5])
    p.close()


def cycle_trace():
    t = fsea.Trace(2048, 2048, m=1)             # a canvas of 4 MiB
    t.frames(data(5, 64), 64, 1, images=False)
    t.close()


def cycle_chain():
    c = fsea.Chain(taps())
    c.run(np.zeros(2 << 19, np.uint8))          # 2^19 pairs: 4 MiB of filtered pairs
    c.close()


@pytest.mark.parametrize("kind,cycle,footprint", [("interp", cycle_interp, 8 * MIB), ("trace", cycle_trace, 4 * MIB),
                                                  ("chain", cycle_chain, 4 * MIB)])
def test_device_memory_comes_back(kind, cycle, footprint):
    """32 cycles of an object whose device footprint is at least 4 MiB.  One object leaked per cycle would lose 32
    footprints; four are allowed for the allocator's granularity."""
    torch.cuda.init()
    cycle()                                     # warm-up: the library's and the runtime's own one-time allocations
    torch.cuda.synchronize()
    free_warm = torch.cuda.mem_get_info()[0]
    for _ in range(CYCLES):
        cycle()
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info()[0]
    print("%s: free after warm-up %d, after %d cycles %d, lost %d bytes (allowed %d)" % (kind, free_warm, CYCLES, free_after,
                                                                                      free_warm - free_after, 4 * footprint))
    assert free_after >= free_warm - 4 * footprint, (kind, free_warm, free_after)
