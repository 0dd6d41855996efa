"""GPU tier: the burst detector (fsea_detect_*, kernels fsea_detect_waves / fsea_detect_slices), the capture object on it
(fsea_capture_*), the nrf_signal_capture block and fsea-signal-capture, against exact integer sums from numpy, the host
detector nrf_signal_detector_process, the scene's state machine written out in tests/capture_ref.py, and the block sequence
the capture replaces (nrf_signal_detector -> nrf_iq_filter -> nut_buffer_append -> nrf_buffer_to_iq_lines) run beside it.

The sums are integers and compared for equality; so are filtered pairs and images, which come from the kernels the block
sequence uses.  The standard deviation follows tests/test_signal_capture_host.py's bound."""
import os
import subprocess

import numpy as np
import pytest

from frequensea_amd import fsea, nrf
from tests import capture_ref as R
from tests.conftest import ROOT
from tests.test_signal_capture_host import TOOL, reference_detector, sd_bound

pytestmark = pytest.mark.gpu

BLOCK_BYTES = [2, 30, 4098, 16384, 16386, 262144]   # under one load; starts at 2 mod 16; the last wave-kernel size; the first
                                                    # slice-kernel size; the scene's
N_BLOCKS = [1, 3, 257]
LINE_PERCENTAGES = [0.2, 0.3, 1.0]


@pytest.fixture(scope="module")
def block():
    """The replay device's block as nrf_device_get_samples_buffer hands it out (offset binary)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "rfdata_all_golden.npz")) as z:
        return np.ascontiguousarray(z["block__raw"] ^ 0x80)


def bits(y):
    return np.ascontiguousarray(y).view(np.uint64)


def numpy_sums(iq, block_bytes, flip):
    b = (iq ^ (0x80 if flip else 0)).reshape(-1, block_bytes).astype(np.uint64)
    return np.stack([b[:, 0::2].sum(axis=1), b.sum(axis=1), (b * b).sum(axis=1)], axis=1)


def device_sums(det, d_in, offset, block_bytes, n_blocks, flip, d_out):
    det.sums_device(d_in.ptr.value + offset, block_bytes, n_blocks, d_out.ptr.value, flip=flip)
    return d_out.download(np.uint64, (n_blocks, 3))


@pytest.mark.parametrize("block_bytes", BLOCK_BYTES)
def test_sums_are_numpys_exact_integers(block_bytes):
    det = fsea.Detect()
    rng = np.random.default_rng(block_bytes)
    iq = rng.integers(0, 256, block_bytes * max(N_BLOCKS), dtype=np.uint8)
    d_in, d_out = fsea.DeviceBuffer(iq.size).upload(iq), fsea.DeviceBuffer(24 * max(N_BLOCKS))
    for n_blocks in N_BLOCKS:
        for flip in (False, True):
            want = numpy_sums(iq[:block_bytes * n_blocks], block_bytes, flip)
            got = device_sums(det, d_in, 0, block_bytes, n_blocks, flip, d_out)
            assert np.array_equal(got, want), (block_bytes, n_blocks, flip)
    d_in.free()
    d_out.free()
    det.close()


@pytest.mark.parametrize("flip", [False, True])
def test_many_blocks_above_the_wave_size_take_one_slice_each(flip):
    """2304 blocks just above the wave kernel's 16 KiB: more blocks than the 8 workgroups per CU the slice kernel aims at
    (2048 on 256 CUs), so each block is one slice and its workgroup stores the sums itself, with no zeroing in front and no
    atomic.  The sums buffer holds ones before the launch: a store that is missing shows.  16400 = 16 * 1025 keeps every
    block start 16-byte aligned; with 16402 block b starts at 2 b mod 16, so heads and tails of every length are summed
    byte by byte under one slice."""
    det = fsea.Detect()
    for block_bytes in (16400, 16402):           # 16402: block b starts at 2 b mod 16, head and tail bytes under one slice
        n_blocks = 2304    # above 8 x the card's CUs (2048 at 256 CUs; up to 288 CUs), else the blocks are cut and added atomically
        iq = np.random.default_rng(block_bytes).integers(0, 256, block_bytes * n_blocks, dtype=np.uint8)
        d_in, d_out = fsea.DeviceBuffer(iq.size).upload(iq), fsea.DeviceBuffer(24 * n_blocks)
        d_out.upload(np.full(3 * n_blocks, 0x0101010101010101, np.uint64))
        got = device_sums(det, d_in, 0, block_bytes, n_blocks, flip, d_out)
        assert np.array_equal(got, numpy_sums(iq, block_bytes, flip)), block_bytes
        d_in.free()
        d_out.free()
    det.close()


def test_blocks_at_the_very_end_of_an_allocation():
    """5 x 4098 bytes that end where the allocation ends still give the right sums for the last block, whose tail is summed
    byte by byte.  The allocator pads an allocation, so a read behind the end would not fault here and would show only if
    it reached a sum; that nothing outside a range is read follows from range_sums itself (bytes one by one up to the
    first and from the last 16-byte boundary, aligned loads only between the two)."""
    det = fsea.Detect()
    n = 5 * 4098
    start = (1 << 20) - n
    assert start % 16 != 0 and (start - 6) % 16 == 0
    start -= 6                                   # a 16-byte aligned base; the allocation ends with the last block
    total = start + n
    d_in, d_out = fsea.DeviceBuffer(total), fsea.DeviceBuffer(24 * 5)
    iq = np.random.default_rng(9).integers(0, 256, total, dtype=np.uint8)
    d_in.upload(iq)
    got = device_sums(det, d_in, start, 4098, 5, False, d_out)
    assert np.array_equal(got, numpy_sums(iq[start:], 4098, False))
    d_in.free()
    d_out.free()
    det.close()


def test_a_block_of_2_to_the_25_bytes_of_255_sums_in_64_bits():
    """The sums of 2^25 bytes of 255 need 41 bits: the reduction across lanes, waves and slices has to be 64 bits wide.  What
    this does not reach is the 32-bit bound of a single lane (16512 dwords of squares): the launch cuts this block into
    2048 slices of 16 KiB, four dwords per lane.  A lane comes near the bound only where one slice is 16 MiB, which takes
    8 workgroups per CU of blocks that large, tens of GiB; the bound is kept by the launch rule (a slice is at most
    16 MiB, a wave's block at most 16 KiB; fsea_detect.hip: DT_MAX_SLICE, DT_WAVE_BLOCK), not shown by a test."""
    det = fsea.Detect()
    n = 1 << 25
    d_in, d_out = fsea.DeviceBuffer(n).upload(np.full(n, 255, np.uint8)), fsea.DeviceBuffer(24)
    got = device_sums(det, d_in, 0, n, 1, False, d_out)
    assert [int(v) for v in got[0]] == [255 << 24, 255 << 25, 65025 << 25]
    got = device_sums(det, d_in, 0, n, 1, True, d_out)          # 255 ^ 0x80 = 127
    assert [int(v) for v in got[0]] == [127 << 24, 127 << 25, 16129 << 25]
    d_in.free()
    d_out.free()
    det.close()


@pytest.mark.parametrize("block_bytes,n_blocks", [(4098, 257), (16384, 64), (262144, 9)])
def test_one_launch_and_one_launch_per_block_and_the_host_form_agree(block, block_bytes, n_blocks):
    """The same recording as one launch of n_blocks and as n_blocks launches of one block (another grid each; a block
    start that is not 16-byte aligned cannot be a launch's base, so those blocks are launched from a copy): the same 24
    bytes per block.  The host form gives the mean of nrf_signal_detector_process bit for bit and its standard deviation
    within the bound."""
    det = fsea.Detect()
    rng = np.random.default_rng(n_blocks)
    iq = np.concatenate([np.roll(block, 2 * int(rng.integers(0, 1000)))[:block_bytes] if k % 3 else
                         rng.integers(0, 256, block_bytes, dtype=np.uint8) for k in range(n_blocks)])
    d_in, d_one, d_out = fsea.DeviceBuffer(iq.size).upload(iq), fsea.DeviceBuffer(block_bytes), fsea.DeviceBuffer(24 * n_blocks)
    whole = device_sums(det, d_in, 0, block_bytes, n_blocks, False, d_out)
    assert np.array_equal(whole, numpy_sums(iq, block_bytes, False))
    for b in range(n_blocks):
        if (b * block_bytes) % 16 == 0:
            one = device_sums(det, d_in, b * block_bytes, block_bytes, 1, False, d_out)
        else:
            d_one.upload(iq[b * block_bytes:(b + 1) * block_bytes])
            one = device_sums(det, d_one, 0, block_bytes, 1, False, d_out)
        assert np.array_equal(one[0], whole[b]), b
    mean, sd = det.run(iq, block_bytes)
    for b in range(0, n_blocks, max(1, n_blocks // 16)):
        want_mean, want_sd = reference_detector(iq[b * block_bytes:(b + 1) * block_bytes])
        assert mean[b] == want_mean, b
        assert abs(sd[b] - want_sd) / want_sd <= sd_bound(block_bytes), b
        assert (mean[b], sd[b]) == fsea.detect_finish(whole[b], block_bytes)
    for buf in (d_in, d_one, d_out):
        buf.free()
    det.close()


def u8_buffer(L, a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return L.nut_buffer_new_u8(a.size // 2, 2, a.ctypes.data)


def filtered_bursts(L, flt, recording, block_bytes, bursts):
    """The block sequence: nrf_iq_filter_process + nrf_iq_filter_get_buffer over the gated blocks in order on `flt`, the
    buffers of a burst joined (what nut_buffer_append does); one float64 array per burst."""
    out = []
    for burst in bursts:
        parts = []
        for b in burst:
            buf = u8_buffer(L, recording[b * block_bytes:(b + 1) * block_bytes])
            L.nrf_iq_filter_process(flt, buf)
            res = L.nrf_iq_filter_get_buffer(flt)
            parts.append(nrf.buffer_to_numpy(L, res))
            L.nut_buffer_free(res)
            L.nut_buffer_free(buf)
        out.append(np.concatenate(parts) if parts else np.empty(0))
    return out


def _lines_equal_the_drawing_function(L, capture, burst, pairs_f64, multiplier, percentages):
    """nrf_signal_capture_get_iq_lines against nrf_buffer_to_iq_lines on the burst's buffer: every pixel equal."""
    a = np.ascontiguousarray(pairs_f64)
    theirs_in = L.nut_buffer_new_f64(a.size // 2, 2, a.ctypes.data)
    for pct in percentages:
        mine, theirs = L.nrf_signal_capture_get_iq_lines(capture, burst, multiplier, pct), L.nrf_buffer_to_iq_lines(theirs_in, multiplier, pct)
        assert mine.contents.length == (256 * multiplier) ** 2 == theirs.contents.length and mine.contents.channels == 1
        x, y = nrf.buffer_to_numpy(L, mine), nrf.buffer_to_numpy(L, theirs)
        assert np.array_equal(x, y) and int(y.max()) > 0, (burst, pct)
        L.nut_buffer_free(mine)
        L.nut_buffer_free(theirs)
    L.nut_buffer_free(theirs_in)


def check_statistics(L, capture, recording, block_bytes, threshold):
    """Every block's statistics against the host detector; every standard deviation further than 1e-6 relative from the
    threshold (NaN aside), so that the bound on it cannot move a block across.  Returns the host detector's values."""
    n_blocks = recording.size // block_bytes
    sds = []
    for b in range(n_blocks):
        want_mean, want_sd = reference_detector(recording[b * block_bytes:(b + 1) * block_bytes])
        mean, sd = L.nrf_signal_capture_get_mean(capture, b), L.nrf_signal_capture_get_standard_deviation(capture, b)
        if np.isnan(want_sd):
            assert np.isnan(sd) and mean == want_mean == 0.0
        else:
            assert mean == want_mean and abs(sd - want_sd) / want_sd <= sd_bound(block_bytes), b
            assert abs(want_sd - threshold) / threshold > 1e-6, (b, want_sd)
        sds.append(want_sd)
    return sds


def test_the_scene_at_its_own_geometry(block):
    """lua/signal-detector.lua: threshold 100, filter (5000000, 200000, 97), ten 262144-byte blocks q q L L L q L q q L."""
    L = nrf.nrf_lib()
    n = block.size
    quiet = R.scale_about_128(block, 2)
    recording = np.concatenate([np.roll(quiet if c == "q" else block, 2 * 37 * k) for k, c in enumerate("qqLLLqLqqL")])
    capture = L.nrf_signal_capture_new(5000000, 200000, 97, 100.0)
    buf = u8_buffer(L, recording)
    assert L.nrf_signal_capture_scan(capture, buf, n // 2) == 3
    L.nut_buffer_free(buf)
    sds = check_statistics(L, capture, recording, n, 100.0)
    assert abs(sds[2] - 140.9) < 0.05 and abs(sds[0] - 70.2) < 0.5, (sds[2], sds[0])
    labels, bursts, state = R.scene(sds, 100.0)
    assert bursts == [[2, 3, 4], [6], [9]] and state == R.CAPTURING
    flt = L.nrf_iq_filter_new(5000000, 200000, 97)
    for k, want in enumerate(filtered_bursts(L, flt, recording, n, bursts)):
        got = L.nrf_signal_capture_get_burst(capture, k)
        assert (got.contents.type, got.contents.length, got.contents.channels) == (nrf.NUT_BUFFER_F64, want.size // 2, 2)
        mine = nrf.buffer_to_numpy(L, got)
        L.nut_buffer_free(got)
        assert np.array_equal(bits(mine), bits(want)), k
        _lines_equal_the_drawing_function(L, capture, k, mine, 4, LINE_PERCENTAGES)
    L.nrf_iq_filter_free(flt)
    L.nrf_signal_capture_free(capture)
    # the same recording through the object itself: where the bursts lie, and the one still open
    cap = fsea.Capture(fsea.lowpass_taps(5000000, 200000, 97))
    assert cap.scan(recording, n, 100.0) == 3
    info = [cap.burst(k) for k in range(3)]
    assert [(i.first_block, i.n_blocks, i.n_pairs, i.open) for i in info] == [(2, 3, 3 * n // 2, 0), (6, 1, n // 2, 0),
                                                                             (9, 1, n // 2, 1)]
    cap.close()


@pytest.fixture(scope="module")
def small(block):
    """Two recordings of five 16384-byte blocks (L loud, q quiet, 0 all zero) and the threshold midway between the two
    levels the host detector measures."""
    bb = 16384
    loud = [np.roll(block, 2 * 101 * k)[:bb] for k in range(10)]
    quiet = [R.scale_about_128(v, 2) for v in loud]
    zero = np.zeros(bb, np.uint8)
    pick = {"L": loud, "q": quiet}
    first = np.concatenate([zero if c == "0" else pick[c][k] for k, c in enumerate("qL0LL")])
    second = np.concatenate([zero if c == "0" else pick[c][5 + k] for k, c in enumerate("Lq0Lq")])
    levels = {c: [reference_detector(v)[1] for v in pick[c]] for c in "Lq"}
    threshold = (min(levels["L"]) + max(levels["q"])) / 2
    assert min(levels["L"]) > threshold * (1 + 1e-6) and max(levels["q"]) < threshold * (1 - 1e-6)
    return bb, first, second, threshold


def test_two_scans_continue_the_open_burst_and_the_filter_tail(small):
    bb, first, second, threshold = small
    L = nrf.nrf_lib()
    capture = L.nrf_signal_capture_new(5000000, 200000, 97, threshold)
    both = np.concatenate([first, second])
    sds = []
    for rec, want_bursts in ((first, 2), (second, 3)):
        buf = u8_buffer(L, rec)
        assert L.nrf_signal_capture_scan(capture, buf, bb // 2) == want_bursts
        L.nut_buffer_free(buf)
        sds += check_statistics(L, capture, rec, bb, threshold)
    labels, bursts, state = R.scene(sds, threshold)
    assert bursts == [[1], [3, 4, 5], [8]] and state == R.DETECTING
    assert labels == ["idle", "start", "end", "start", "captured", "captured", "end", "idle", "start", "end"]
    flt = L.nrf_iq_filter_new(5000000, 200000, 97)
    for k, want in enumerate(filtered_bursts(L, flt, both, bb, bursts)):
        got = L.nrf_signal_capture_get_burst(capture, k)
        mine = nrf.buffer_to_numpy(L, got)
        L.nut_buffer_free(got)
        assert np.array_equal(bits(mine), bits(want)), k
        _lines_equal_the_drawing_function(L, capture, k, mine, 2, LINE_PERCENTAGES)
    L.nrf_iq_filter_free(flt)
    L.nrf_signal_capture_free(capture)
    # the object itself: the open flag after each scan, block indices that count across the scans, the device form, reset
    cap = fsea.Capture(fsea.lowpass_taps(5000000, 200000, 97))
    assert cap.scan(first, bb, threshold) == 2
    assert [(cap.burst(k).first_block, cap.burst(k).n_blocks, cap.burst(k).open) for k in range(2)] == [(1, 1, 0), (3, 2, 1)]
    d_in = fsea.DeviceBuffer(second.size).upload(second)
    assert cap.scan_device(d_in.ptr.value, bb, 5, threshold) == 3
    assert [(cap.burst(k).first_block, cap.burst(k).n_blocks, cap.burst(k).open) for k in range(3)] == [(1, 1, 0), (3, 3, 0),
                                                                                                      (8, 1, 0)]
    mean, sd = cap.stats()
    assert mean.size == 5 and np.isnan(sd[2]) and mean[2] == 0.0
    ref = fsea.Fir(fsea.lowpass_taps(5000000, 200000, 97))
    want = [ref.run_u8(np.concatenate([both[b * bb:(b + 1) * bb] for b in burst])) for burst in bursts]
    for k in range(3):
        assert np.array_equal(cap.burst_pairs(k).view(np.uint64), want[k].view(np.uint64)), k
    d_img = fsea.DeviceBuffer(65536)
    cap.burst_lines_device(1, 1, 1000, d_img.ptr.value)
    assert np.array_equal(d_img.download(np.uint8, (256, 256)), cap.burst_lines(1, 1, 1000))
    with pytest.raises(fsea.FseaError):
        cap.burst(3)
    with pytest.raises(fsea.FseaError):
        cap.burst_lines(1, 1, 3 * bb // 2 + 1)
    cap.reset()
    assert cap.n_bursts == 0 and cap.scan(second, bb, threshold) == 2 and cap.burst(0).first_block == 0
    ref.reset()
    assert np.array_equal(cap.burst_pairs(0).view(np.uint64), ref.run_u8(second[:bb]).view(np.uint64))
    for obj in (d_in, d_img):
        obj.free()
    ref.close()
    cap.close()


def test_the_tool_prints_the_states_and_writes_the_frames(small, tmp_path):
    from PIL import Image
    bb, first, second, threshold = small
    both = np.concatenate([first, second, first[:100]])            # a trailing partial block is ignored
    rec, out = tmp_path / "recording.raw", tmp_path / "out"
    both.tofile(str(rec))
    out.mkdir()
    r = subprocess.run([TOOL, "--block-bytes", str(bb), "--multiplier", "1", "--step", "0.25", "--threshold", repr(threshold),
                        "--out-dir", str(out), str(rec)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    printed = r.stdout.splitlines()
    assert len(printed) == 10 + 12 and all(ln.startswith("Written ") for ln in printed[10:])   # write_gray_png's own lines
    lines = [ln.split() for ln in printed[:10]]
    sds = [reference_detector(both[b * bb:(b + 1) * bb])[1] for b in range(10)]
    labels, bursts, _ = R.scene(sds, threshold)
    assert [ln[0] for ln in lines] == [str(b) for b in range(10)] and [ln[3] for ln in lines] == labels
    for b, ln in enumerate(lines):
        if np.isnan(sds[b]):
            assert "nan" in ln[2].lower()
        else:
            assert abs(float(ln[2]) - sds[b]) / sds[b] <= sd_bound(bb)
    assert sorted(os.listdir(str(out))) == ["burst-%03d-%04d.png" % (k, f) for k in range(3) for f in range(4)]
    L = nrf.nrf_lib()
    flt = L.nrf_iq_filter_new(5000000, 200000, 97)
    for k, want in enumerate(filtered_bursts(L, flt, both, bb, bursts)):
        buf = L.nut_buffer_new_f64(want.size // 2, 2, np.ascontiguousarray(want).ctypes.data)
        p = 0.0
        for f in range(4):
            img = L.nrf_buffer_to_iq_lines(buf, 1, np.float32(p))
            got = np.asarray(Image.open(str(out / ("burst-%03d-%04d.png" % (k, f)))))
            assert got.dtype == np.uint8 and np.array_equal(got.ravel(), nrf.buffer_to_numpy(L, img)), (k, f)
            assert f == 0 or got.any()
            L.nut_buffer_free(img)
            p += 0.25
        L.nut_buffer_free(buf)
    L.nrf_iq_filter_free(flt)
