"""GPU tier: the frequency-shifted FIR kernel (fsea_fir_u8_shifted_*, kernel fsea_shift_fir_u8), the chain object on it
(fsea_chain_*) and the nrf_iq_chain block, against the f64 restatement of tests/test_iq_chain_host.py (pinned there to the
reference's own recorded dvbt.lua outputs), the reference's outputs themselves, and the block sequence the chain replaces
(nrf_freq_shifter -> nrf_iq_filter -> nrf_buffer_to_iq_points / _lines) run beside it.

Tolerance: MAX_ABS and MAX_REL of tests/test_gpu_fir.py, whose derivation covers inputs in [-0.5, 1.5], the shifter's
range.  The rotation adds one input-side term: a float phasor evaluated from a phase reduced in double is off by a few
2^-24, times |u8 / 256| < 1, times sum |c| < 2 -- under 1e-6 absolute.  Images and everything the chain shares a kernel
with are compared for equality."""
import ctypes
import threading
import time

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests.test_fir_host import GOLDEN, fir_reference
from tests.test_gpu_fir import MAX_ABS, _replay_device, check, random_taps, u8_to_complex
from tests.test_iq_chain_host import shifted_fir_reference

pytestmark = pytest.mark.gpu

LENGTHS = [1, 21, 51, 97, 512]
COUNTS = [1, 7, 2047, 2048, 2049, 131072, (1 << 22) + 13]
CYCLES = [0.0, 50e3 / 5e6, -1.2e6 / 10e6, 0.4999]
PHASES = [0.0, 0.75, 12345.678]
SCENE_FILTERS = [(200e3, 21), (200e3, 51), (200e3, 97)]
LINE_PERCENTAGES = [0.2, 0.3, 1.0]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def block():
    """The replay device's block as nrf_device_get_samples_buffer hands it out (offset binary)."""
    with np.load(GOLDEN.replace("iq_filter_golden", "rfdata_all_golden")) as z:
        return np.ascontiguousarray(z["block__raw"] ^ 0x80)


def bits(y):
    return np.ascontiguousarray(y).view(np.uint64)


def buffer_pairs(L, buf):
    v = nrf.buffer_to_numpy(L, buf)
    return v[0::2] + 1j * v[1::2]


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("flip", [0, 1])
def test_shifted_sizes_against_the_restatement(L, flip):
    """Host and device forms, every sample of every (n, cycles_per_sample, phase0_cycles) checked."""
    c = random_taps(L, L)
    fir = fsea.Fir(c)
    rng = np.random.default_rng(2000 + L)
    d_in, d_out = fsea.DeviceBuffer(2 * max(COUNTS)), fsea.DeviceBuffer(8 * max(COUNTS))
    for n in COUNTS:
        iq = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        d_in.upload(iq)
        for cps in CYCLES:
            for phase0 in PHASES:
                want, _ = shifted_fir_reference(iq, flip, cps, phase0, c)
                fir.reset()
                got = fir.run_u8_shifted(iq, cps, phase0, flip=bool(flip))
                check(got, want, ("host", L, n, flip, cps, phase0))
                fir.reset()
                fir.run_shifted_device(d_in.ptr.value, n, d_out.ptr.value, cps, phase0, flip=bool(flip))
                got_d = d_out.download(np.complex64, n)
                check(got_d, want, ("device", L, n, flip, cps, phase0))
                assert np.array_equal(bits(got), bits(got_d)), (L, n, flip, cps, phase0)
    d_in.free()
    d_out.free()
    fir.close()


@pytest.mark.parametrize("L", [21, 97, 512])
def test_a_stream_cut_anywhere_is_the_one_call_result_bit_for_bit(L):
    """2^20 samples in calls of random lengths, each continued with sample_offset = the samples consumed so far: the
    phasor of a sample depends on its stream position alone, the accumulation order is fixed, so the pieces are the
    one-call result bit for bit.  Host and device forms; two runs of the device form are bit-identical."""
    n = 1 << 20
    cps, phase0 = -1.2e6 / 10e6, 0.75
    c = random_taps(L, 5 * L)
    rng = np.random.default_rng(L)
    iq = rng.integers(0, 256, 2 * n, dtype=np.uint8)
    cuts = [1, 3, max(L - 2, 1), 5000, 8, 2048, 17, 70001, 1, L // 2 + 1] + list(rng.integers(1, 200000, 6))
    cuts = [int(k) for k in cuts]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    whole = fsea.Fir(c)
    want = whole.run_u8_shifted(iq, cps, phase0, flip=True)
    check(want, shifted_fir_reference(iq, 1, cps, phase0, c)[0], L)
    parts = fsea.Fir(c)
    got, pos = [], 0
    for k in cuts:
        got.append(parts.run_u8_shifted(iq[2 * pos:2 * (pos + k)], cps, phase0, sample_offset=pos, flip=True))
        pos += k
    assert np.array_equal(bits(np.concatenate(got)), bits(want))
    # the device form: pieces that start on 8-sample boundaries of the input buffer (16-byte alignment), each written at its
    # own place in the output
    d_in, d_out = fsea.DeviceBuffer(2 * n), fsea.DeviceBuffer(8 * n)
    d_in.upload(iq)
    runs = []
    for _ in range(2):
        whole.reset()
        whole.run_shifted_device(d_in.ptr.value, n, d_out.ptr.value, cps, phase0, flip=True)
        runs.append(d_out.download(np.complex64, n))
    assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.array_equal(bits(runs[0]), bits(want))
    parts.reset()
    pos = 0
    for k in [8, 4096, 70000, 8 * 12345, 2048 + 8]:
        parts.run_shifted_device(d_in.ptr.value + 2 * pos, k, d_out.ptr.value + 8 * pos, cps, phase0, sample_offset=pos,
                                 flip=True)
        pos += k
    parts.run_shifted_device(d_in.ptr.value + 2 * pos, n - pos, d_out.ptr.value + 8 * pos, cps, phase0, sample_offset=pos,
                             flip=True)
    assert np.array_equal(bits(d_out.download(np.complex64, n)), bits(want))
    d_in.free()
    d_out.free()
    whole.close()
    parts.close()


@pytest.mark.parametrize("how", ["sample_offset", "phase0_cycles"])
def test_a_phase_of_1e9_consumed_samples_stays_inside_the_tolerance(how):
    """50 kHz at 5 MHz after 10^9 samples: 10^7 cycles.  A float phase (or a float product m * delta) is off by whole
    radians here; the phase reduced in double is not.  The expected phase is exact integer arithmetic: delta = 1 / 100."""
    n, consumed = 131072, 10 ** 9
    c = random_taps(97, 11)
    iq = np.random.default_rng(4).integers(0, 256, 2 * n, dtype=np.uint8)
    x = u8_to_complex(iq, 0)
    turns = ((consumed + np.arange(n)) % 100) / 100.0
    want, _ = fir_reference(x * np.exp(2j * np.pi * turns) + (0.5 + 0.5j), c)
    fir = fsea.Fir(c)
    if how == "sample_offset":
        got = fir.run_u8_shifted(iq, 50e3 / 5e6, 0.0, sample_offset=consumed)
    else:
        got = fir.run_u8_shifted(iq, 50e3 / 5e6, consumed * (50e3 / 5e6))
    check(got, want, how)
    fir.close()


def test_dvbt_chain_against_restatement_reference_and_block_sequence(gold, block, tmp_path):
    """lua/dvbt.lua: shifter -> filter(5e6, 60e3, 97) on three replayed blocks.  2N pairs per call (N rotated, N zero); the
    chain against the f64 restatement, the reference's recorded outputs, and nrf_freq_shifter -> nrf_iq_filter beside it
    (2 MAX_ABS: both sides carry the kernel's error).  The images are those of the drawing functions on the chain's own
    buffer, byte for byte."""
    L = nrf.nrf_lib()
    raw = block ^ 0x80
    dev = _replay_device(L, tmp_path, raw)
    shift = int(gold["dvbt__shift"])
    chain = L.nrf_iq_chain_new(5000000, 60000, 97)
    L.nrf_iq_chain_set_shifter(chain, shift)
    shifter = L.nrf_freq_shifter_new(shift, 5000000)
    flt = L.nrf_iq_filter_new(5000000, 60000, 97)
    c = gold["taps__5000000_60000_97"]
    idx, tail, n = gold["dvbt__index"], None, block.size // 2
    for step in range(3):
        L.nrf_device_step(dev)
        time.sleep(0.06)
        buf = L.nrf_device_get_samples_buffer(dev)
        assert np.array_equal(nrf.buffer_to_numpy(L, buf), block)
        L.nrf_iq_chain_process(chain, buf)
        out = L.nrf_iq_chain_get_buffer(chain)
        assert out.contents.length == 2 * n and out.contents.channels == 2 and out.contents.type == nrf.NUT_BUFFER_F64
        y = buffer_pairs(L, out)
        want, tail = shifted_fir_reference(block, 0, shift / 5e6, 0.0, c, tail, offset=step * n, n_zero=n)
        check(y, want, ("dvbt", step))
        ref = gold["dvbt__out"][step]
        check(y[idx], ref[:, 0] + 1j * ref[:, 1], ("dvbt reference", step))
        L.nrf_freq_shifter_process(shifter, buf)
        sb = L.nrf_freq_shifter_get_buffer(shifter)
        L.nrf_iq_filter_process(flt, sb)
        fb = L.nrf_iq_filter_get_buffer(flt)
        z = buffer_pairs(L, fb)
        assert z.shape == y.shape
        err = float(np.max(np.abs(y - z)))
        print("dvbt step %d: chain against the block sequence, max |delta| %.3e" % (step, err))
        assert err <= 2 * MAX_ABS, (step, err)
        _images_equal_the_drawing_functions(L, chain, out, (4,), LINE_PERCENTAGES)
        for b in (out, sb, fb, buf):
            L.nut_buffer_free(b)
    L.nrf_iq_chain_free(chain)
    L.nrf_iq_filter_free(flt)
    L.nrf_freq_shifter_free(shifter)
    L.nrf_device_free(dev)


def _images_equal_the_drawing_functions(L, chain, out, multipliers, percentages):
    """nrf_iq_chain_get_iq_points / _lines against nrf_buffer_to_iq_points / _lines on `out`, the buffer
    nrf_iq_chain_get_buffer returned for the same call: every pixel equal."""
    mine, theirs = L.nrf_iq_chain_get_iq_points(chain), L.nrf_buffer_to_iq_points(out)
    a, b = nrf.buffer_to_numpy(L, mine), nrf.buffer_to_numpy(L, theirs)
    assert a.size == 65536 and np.array_equal(a, b) and int(b.sum()) > 0
    L.nut_buffer_free(mine)
    L.nut_buffer_free(theirs)
    for m in multipliers:
        for pct in percentages:
            mine, theirs = L.nrf_iq_chain_get_iq_lines(chain, m, pct), L.nrf_buffer_to_iq_lines(out, m, pct)
            assert mine.contents.length == (256 * m) ** 2 == theirs.contents.length and mine.contents.channels == 1
            a, b = nrf.buffer_to_numpy(L, mine), nrf.buffer_to_numpy(L, theirs)
            assert np.array_equal(a, b) and int(b.max()) > 0, (m, pct)
            L.nut_buffer_free(mine)
            L.nut_buffer_free(theirs)


@pytest.mark.parametrize("cutoff,length", SCENE_FILTERS)
def test_unshifted_chain_is_nrf_iq_filter_bit_for_bit_and_its_images_are_exact(block, cutoff, length):
    """lua/iq-tex-filtered.lua and friends: no shifter.  Same kernel, same order: get_buffer is nrf_iq_filter's, bit for
    bit, over three blocks (the tail carries); points and lines (m = 4; 0.2, 0.3, 1.0) equal the drawing functions'."""
    L = nrf.nrf_lib()
    chain = L.nrf_iq_chain_new(5000000, int(cutoff), length)
    flt = L.nrf_iq_filter_new(5000000, int(cutoff), length)
    rng = np.random.default_rng(length)
    for step in range(3):
        data = block if step == 0 else np.ascontiguousarray(np.roll(block, 2 * int(rng.integers(1, 1000))))
        buf = L.nut_buffer_new_u8(data.size // 2, 2, data.ctypes.data)
        L.nrf_iq_chain_process(chain, buf)
        L.nrf_iq_filter_process(flt, buf)
        out, want = L.nrf_iq_chain_get_buffer(chain), L.nrf_iq_filter_get_buffer(flt)
        assert out.contents.length == data.size // 2 == want.contents.length
        assert np.array_equal(nrf.buffer_to_numpy(L, out).view(np.uint64), nrf.buffer_to_numpy(L, want).view(np.uint64))
        _images_equal_the_drawing_functions(L, chain, out, (4,), LINE_PERCENTAGES)
        for b in (out, want, buf):
            L.nut_buffer_free(b)
    L.nrf_iq_chain_free(chain)
    L.nrf_iq_filter_free(flt)


def test_set_shifter_in_mid_sequence_restarts_the_phase_and_keeps_the_tail(block):
    L = nrf.nrf_lib()
    c = fsea.lowpass_taps(5e6, 60e3, 97)
    chain = L.nrf_iq_chain_new(5000000, 60000, 97)
    assert not L.nrf_iq_chain_get_buffer(chain) and not L.nrf_iq_chain_get_iq_points(chain)     # NULL before any process
    assert not L.nrf_iq_chain_get_iq_lines(chain, 4, 0.2)
    n, tail = 4000, None
    plan = [(None, 0), (None, 0), (50000, 0), (50000, n), (-1200000, 0), (-1200000, n), (-1200000, 2 * n)]
    last = None
    for step, (offset_hz, consumed) in enumerate(plan):
        if offset_hz != last and offset_hz is not None:
            L.nrf_iq_chain_set_shifter(chain, offset_hz)
        last = offset_hz
        data = np.ascontiguousarray(block[2 * n * step:2 * n * (step + 1)])
        buf = L.nut_buffer_new_u8(n, 2, data.ctypes.data)
        L.nrf_iq_chain_process(chain, buf)
        out = L.nrf_iq_chain_get_buffer(chain)
        if offset_hz is None:
            want, tail = fir_reference(u8_to_complex(data, 0), c, tail)
        else:
            want, tail = shifted_fir_reference(data, 0, offset_hz / 5e6, 0.0, c, tail, offset=consumed, n_zero=n)
        check(buffer_pairs(L, out), want, (step, offset_hz))
        L.nut_buffer_free(out)
        L.nut_buffer_free(buf)
    L.nrf_iq_chain_free(chain)


def test_f64_input_takes_the_host_staged_path(block):
    """F64 buffers, with and without a shifter, mixed with U8 buffers in one chain: one filter state."""
    L = nrf.nrf_lib()
    c = fsea.lowpass_taps(5e6, 200e3, 51)
    chain = L.nrf_iq_chain_new(5000000, 200000, 51)
    rng = np.random.default_rng(6)
    tail, consumed = None, 0
    for step, (kind, shifted) in enumerate([("u8", False), ("f64", False), ("f64", True), ("u8", True), ("f64", True)]):
        n = [3000, 20, 4097, 1, 2500][step]
        if step == 2:
            L.nrf_iq_chain_set_shifter(chain, 50000)
        if kind == "u8":
            data = rng.integers(0, 256, 2 * n, dtype=np.uint8)
            buf = L.nut_buffer_new_u8(n, 2, data.ctypes.data)
            x = u8_to_complex(data, 0)
        else:
            data = rng.uniform(0.0, 1.0, 2 * n)
            buf = L.nut_buffer_new_f64(n, 2, data.ctypes.data)
            x = data[0::2] + 1j * data[1::2]
        if shifted:
            turns = (consumed + np.arange(n)) * (50000 / 5e6)
            x = np.concatenate([x * np.exp(2j * np.pi * turns) + (0.5 + 0.5j), np.zeros(n, dtype=np.complex128)])
            consumed += n
        L.nrf_iq_chain_process(chain, buf)
        out = L.nrf_iq_chain_get_buffer(chain)
        want, tail = fir_reference(x, c, tail)
        check(buffer_pairs(L, out), want, (step, kind, shifted))
        _images_equal_the_drawing_functions(L, chain, out, (1,), (1.0,))
        L.nut_buffer_free(out)
        L.nut_buffer_free(buf)
    L.nrf_iq_chain_free(chain)


def test_two_chains_on_two_threads_keep_their_own_state(block):
    cs = [random_taps(97, 1), random_taps(51, 2)]
    shifts = [50e3 / 5e6, None]
    rng = np.random.default_rng(9)
    streams = [rng.integers(0, 256, 2 * 300000, dtype=np.uint8) for _ in cs]
    cuts = [1000, 7, 50000, 20, 123456, 1, 125516]
    results, images = [None, None], [None, None]

    def run(k):
        chain = fsea.Chain(cs[k])
        parts, pos = [], 0
        for n in cuts:
            st = None if shifts[k] is None else fsea.Chain.stage(cycles_per_sample=shifts[k], sample_offset=pos)
            res = chain.run(streams[k][2 * pos:2 * (pos + n)], st, points=True, pairs=True)
            parts.append(res["pairs"])
            pos += n
        results[k], images[k] = np.concatenate(parts), res["points"]
        chain.close()

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    check(results[0], shifted_fir_reference(streams[0], 0, shifts[0], 0.0, cs[0])[0], 0)
    check(results[1], fir_reference(u8_to_complex(streams[1], 0), cs[1])[0], 1)
    draw = fsea.IqDraw()
    for k in range(2):
        assert np.array_equal(images[k], draw.points(results[k][-cuts[-1]:]))
    draw.close()


@pytest.mark.parametrize("shifted,n_zero", [(False, 0), (True, 0), (True, 131072)])
def test_batched_device_form_equals_single_calls_byte_for_byte(block, shifted, n_zero):
    """8 blocks of one stream in one fsea_chain_run_device call -> 8 points images, 8 lines images (m = 4, the first 0.2 of
    each frame) and the pairs, against 8 host runs of a second chain: every byte."""
    frames, n, m = 8, block.size // 2, 4
    c = fsea.lowpass_taps(5e6, 60e3, 97)
    rng = np.random.default_rng(12)
    stream = np.concatenate([np.roll(block, 2 * int(rng.integers(0, 5000))) for _ in range(frames)])
    per = n + n_zero
    n_line = per // 5
    cps = 50e3 / 5e6 if shifted else None
    single = fsea.Chain(c)
    want = []
    for f in range(frames):
        st = fsea.Chain.stage(cycles_per_sample=cps, sample_offset=f * n, n_zero=n_zero) if shifted else None
        want.append(single.run(stream[2 * n * f:2 * n * (f + 1)], st, points=True, lines_m=m, n_line_points=n_line, pairs=True))
    single.close()
    pts, lns, prs = frames * 65536, frames * (256 * m) ** 2, frames * per * 8
    d_in, d_out = fsea.DeviceBuffer(stream.nbytes), fsea.DeviceBuffer(pts + lns + prs)
    d_in.upload(stream)
    batched = fsea.Chain(c)
    st = fsea.Chain.stage(cycles_per_sample=cps, n_zero=n_zero) if shifted else None
    base = d_out.ptr.value
    batched.run_device(d_in.ptr.value, n, frames, st, d_points=base, d_lines=base + pts, lines_m=m, n_line_points=n_line,
                       d_pairs=base + pts + lns)
    got_p = d_out.download(np.uint8, pts).reshape(frames, 256, 256)
    got_l = d_out.download(np.uint8, lns, pts).reshape(frames, 256 * m, 256 * m)
    got_y = d_out.download(np.complex64, frames * per, pts + lns).reshape(frames, per)
    for f in range(frames):
        assert np.array_equal(bits(got_y[f]), bits(want[f]["pairs"])), f
        assert np.array_equal(got_p[f], want[f]["points"]) and np.array_equal(got_l[f], want[f]["lines"]), f
        assert int(got_l[f].max()) > 0
    assert batched.n_pairs == per
    batched.close()
    d_in.free()
    d_out.free()
