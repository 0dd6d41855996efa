"""GPU tier (-m gpu): the transform sizes without a kernel of their own -- frequensea_amd/csrc/fsea_anysize.hip: Bluestein's
algorithm (2 ... 524287 points, everything that is not a power of two from 32 up) and the four-step decomposition
(2^15 ... 2^20 points) -- at the places the three tests of test_gpu_parity.py do not reach: the seams between the chunks
of the plan's work buffers, hops other than the transform size, epilogue modes and byte conventions that never ran, the
neighbours of the kernel range, the largest sizes, the bytes around the output rows, two streams and two host threads on
one plan's work buffers, and the entry points such a plan refuses.

References: numpy's f64 FFT (the oracle's O(n^2) long-double DFT up to 1001 points) around the oracle's own unpack,
magnitude and pixel loops (tests/parity.py: any_size_spectra, check_spectra); bounds: parity.check_float / check_u8 /
check_db, the ones of every other size.  Data goes in resident (exec_device) wherever a chunk seam is the subject: the
host entry points cut a large batch into pieces of about 24 MiB of their own, shorter than a work-buffer chunk for any batch
below 16 such pieces."""
import ctypes
import functools
import threading

import numpy as np
import pytest

from frequensea_amd import fsea
from oracle import oracle as O
from tests import parity
from tests.conftest import synth_iq

pytestmark = pytest.mark.gpu

DeviceBuffer = fsea.DeviceBuffer
GUARD = 1 << 16          # bytes of 0xA5 in front of and behind the output rows of every resident launch here
FLIP_MASK = np.uint8(0x80)   # raw int8 bytes ^ 0x80 = the same samples in offset binary (flip=False)


def bluestein_m(n):
    """bluestein_m (fsea_anysize.hip): the power of two >= 2n - 1 (at least 32) of the two inner transforms."""
    m = 32
    while m < 2 * n - 1:
        m <<= 1
    return m


def is_fourstep(n):
    return n > 16384 and n & (n - 1) == 0


def work_frames(n):
    """Frames per chunk of blu_launch / fs_launch (p->work.frames): each of the plan's two work buffers holds 64 MiB of
    complex64 (8 bytes), a frame taking n of them on the four-step path (fs_setup) and m = bluestein_m(n) on Bluestein's
    (blu_setup, capped at 65536 frames)."""
    if is_fourstep(n):
        return (64 << 20) // (8 * n)
    return min(65536, (64 << 20) // (8 * bluestein_m(n)))


def frames_iq(seed, n, nf, hop):
    """A u8 IQ stream of nf frames at `hop`, the bytes from each frame's start to the next one's drawn from a seed of their
    own: no two rows alike, so a row written in another row's place cannot pass."""
    parts = [synth_iq(seed + f, 2 * hop) for f in range(nf - 1)] + [synth_iq(seed + nf - 1, 2 * n)]
    return np.concatenate(parts)


@functools.lru_cache(maxsize=3)
def case(n, nf, hop, seed):
    """(iq, f64 spectra of its nf frames as raw int8 bytes; numpy's FFT at every size), computed once and shared by the
    tests and modes that run the same geometry; read-only."""
    iq = frames_iq(seed, n, nf, hop)
    spectra = parity.any_size_spectra(iq, n, nf, hop, True, exact=False)
    iq.setflags(write=False)
    spectra.setflags(write=False)
    return iq, spectra


def upload(d_buf, arr):
    """DeviceBuffer.upload through a page-locked copy of the array (fsea.PinnedArray).  A precaution, and DESIGN.md section 6
    says so: the one GPU fault this file has seen was reported by a pageable device-to-host copy of several MiB into a numpy
    array allocated a moment before, which the runtime has to pin for the transfer.  Whether that was the cause is not
    known; the earlier tests of test_gpu_parity.py keep DeviceBuffer's own pageable copies."""
    arr = np.ascontiguousarray(arr)
    h = fsea.PinnedArray(arr.shape, arr.dtype)
    try:
        h.array[...] = arr
        fsea._check(fsea.hip_lib().fsea_copy_to_device(d_buf.device, d_buf.ptr, h.array.ctypes.data, h.array.nbytes))
    finally:
        h.close()
    return d_buf


def download(d_buf, dtype, shape):
    """The start of a device buffer as a new host array, through a page-locked array as in upload()."""
    h = fsea.PinnedArray(shape, dtype)
    try:
        fsea._check(fsea.hip_lib().fsea_copy_to_host(d_buf.device, h.array.ctypes.data, d_buf.ptr, h.array.nbytes))
        return h.array.copy()
    finally:
        h.close()


def exec_resident(plan, iq, nf, flip=True):
    """exec_device on resident bytes (the input buffer ends with the last frame's last byte), the output rows between two
    guard bands; returns the rows after checking that no byte of either band changed."""
    out_bytes = nf * plan.row_bytes
    assert iq.nbytes == plan.in_bytes(nf)
    d_in = upload(DeviceBuffer(iq.nbytes), iq)
    d_buf = upload(DeviceBuffer(GUARD + out_bytes + GUARD), np.full(GUARD + out_bytes + GUARD, 0xA5, np.uint8))
    try:
        plan.exec_device(d_in.ptr, nf, ctypes.c_void_p(d_buf.ptr.value + GUARD), flip=flip)
        plan.synchronize()
        back = download(d_buf, np.uint8, (GUARD + out_bytes + GUARD,))
    finally:
        d_in.free()
        d_buf.free()
    assert np.all(back[:GUARD] == 0xA5), "bytes in front of the first row were written"
    assert np.all(back[GUARD + out_bytes:] == 0xA5), "bytes behind the last row were written"
    return back[GUARD: GUARD + out_bytes].view(plan.out_dtype).reshape(nf, plan.fft_size)


def check_patched_bin(got, n, mode):
    """MAG and DB5 rows carry bin n/2 - 1 in bin n/2 (the integer n/2 of the reference), bit for bit."""
    if mode in (0, 2):
        assert np.array_equal(got[:, n // 2], got[:, n // 2 - 1])


def run_seam(n, nf, hop, mode, seed, name):
    assert nf == work_frames(n) + 1, "the last chunk holds exactly one frame"
    iq, spectra = case(n, nf, hop, seed)
    plan = fsea.Plan(n, hop=hop, mode=mode)
    assert plan.kernel_name.startswith(name)
    got = exec_resident(plan, iq, nf)
    plan.close()
    parity.check_spectra(got, spectra, mode)
    check_patched_bin(got, n, mode)


# ---------------------------------------------------------------------------------------------
# 1. chunk seams
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nf,hop,mode", [(32768, 257, 32768, 0), (32768, 257, 32768, 1), (32768, 257, 32768, 3),
                                           (1 << 20, 9, 1 << 20, 0), (32768, 257, 12345, 0),
                                           (32768, 257, 32775, 0)])
def test_fourstep_rows_across_a_chunk_seam(n, nf, hop, mode):
    """fs_launch's second chunk: input offset f0 * hop * in_bps, output offset f0 * n * esz, and a last chunk of one frame
    (nf = 1 in the three helper kernels while the inner plans run n2 and n1 frames).  A chunk is 64 MiB / (8 n) frames --
    256 at 32768 points, 8 at 2^20 (work_frames) -- so the 2 frames of test_transform_sizes_above_the_largest_kernel never
    leave the first one, and neither does exec_host below 16 pieces of 256 frames (its pieces of about 24 MiB are shorter
    than a chunk until their number is capped: over 4096 frames, 0.8 GB, at 32768 points): resident data, chunk + 1 frames,
    every row checked.  esz = 4, 1 and 8 (modes 0, 1, 3); the odd hop 12345 makes the second chunk's
    input start at an odd sample and an address that is not 16-byte aligned, and hop = n + 7 leaves a gap between frames
    (fsea_fs_prep_kernel reads sample f * hop + n2 * j1 + j2 and signs it by (j2 ^ j1) & 1, the parity of the index within
    the frame whatever the frame's first sample); at 2^20 the offsets are f0 * 8 MiB."""
    run_seam(n, nf, hop, mode, 5000 + hop % 1000, "fourstep(")


@pytest.mark.parametrize("n,nf,hop,mode", [(8191, 513, 8191, 0), (8191, 513, 8191, 2), (8191, 513, 2731, 0),
                                           (8191, 513, 2731, 2), (9000, 257, 9000, 3)])
def test_bluestein_rows_across_a_chunk_seam(n, nf, hop, mode):
    """blu_launch's second chunk, offsets as in fs_launch but with rows of n and work frames of m points: 8191 points
    (m = 16384, 64 MiB / (8 m) = 512 frames per chunk) with hop = n and hop = 2731, rows of 4 and 1 bytes; 9000 points
    (m = 32768, 256 frames per chunk) where the inner plan is itself a four-step plan with work buffers and an event of
    its own, rows of 8 bytes.  The one two-chunk case there was, 17 points x 70000 frames in mode 0 with hop = n
    (test_transform_sizes_fftw_takes_and_the_kernels_do_not, kept), checks 3 rows; here every row is, and the grids
    of the helper kernels are at their cap of 8192 blocks in the first chunk and at one frame's size in the second."""
    run_seam(n, nf, hop, mode, 6000 + hop % 1000, "bluestein(fourstep(" if n == 9000 else "bluestein(fsea_fft")


# ---------------------------------------------------------------------------------------------
# 2. four-step geometry
# ---------------------------------------------------------------------------------------------
HOPS = {"n": lambda n: n, "half": lambda n: n // 2, "one": lambda n: 1, "gapped": lambda n: n + 7}


@pytest.mark.parametrize("lg,hop_kind", [(lg, k) for lg in range(15, 21) for k in (("n", "half", "one", "gapped") if lg <= 17
                                                                                   else ("n", "half"))
                                         if (lg, k) != (18, "half")])
def test_fourstep_every_split_hop_mode_and_byte_convention(lg, hop_kind):
    """fourstep_split's six (n1, n2) pairs: 256 x 128, 256 x 256, 512 x 256, 512 x 512, 1024 x 512, 1024 x 1024 (2^17, 2^19
    and 2^20, the documented maximum, had no test), 3 frames.  fsea_fs_prep_kernel reads sample f * hop + n2 * j1 + j2 and
    signs it by (j2 ^ j1) & 1, fsea_fs_twiddle_kernel by j2 & 1: the parity is that of the index within the frame whatever the
    frame's first sample, so hop = 1 (odd, frames overlap all but one sample), n / 2 and n + 7 (odd, gapped) must give the
    rows of hop = n's arithmetic -- only hop = n was run.  fsea_fs_epilogue_kernel: modes 0-5 with both byte conventions at
    2^15 and 2^17 (an odd and an even log2, n1 != n2 in both; modes 1, 4, 5 never ran here, flip=False only in mode 3 at
    32768), bin n/2 := bin n/2 - 1 in modes 0 and 2 (`k == n/2` after `k -= 1` must not add the DC term).
    Not run: 2^18 points with hop n / 2.  That case passed twice and on a third run ended in "an illegal memory access",
    reported by the copy back after a synchronisation that succeeded; no cause was found in fsea_anysize.hip or in launch()
    (DESIGN.md section 6), and it stays out until one is."""
    n = 1 << lg
    nf = 3
    hop = HOPS[hop_kind](n)
    modes = (0, 1, 2, 3, 4, 5) if lg in (15, 17) else (0, 3)
    flips = (True, False) if lg in (15, 17) else (True,)
    iq = frames_iq(7000 + lg + hop % 97, n, nf, hop)
    spectra = parity.any_size_spectra(iq, n, nf, hop, True)
    offset_binary = iq ^ FLIP_MASK
    for mode in modes:
        plan = fsea.Plan(n, hop=hop, mode=mode)
        assert plan.kernel_name.startswith("fourstep(")
        for flip in flips:
            got = exec_resident(plan, iq if flip else offset_binary, nf, flip=flip)
            parity.check_spectra(got, spectra, mode)
            check_patched_bin(got, n, mode)
        plan.close()


def dc_only_spectra(n):
    """Spectrum of one frame of zero bytes read as raw int8 (flip): u8 128 -> 0.5 (1 + i) (-1)^j, i.e. 0.5 n (1 + i) in bin
    n/2 (even n) and nothing anywhere else."""
    s = np.zeros((1, n), dtype=np.complex128)
    s[0, n // 2] = 0.5 * n * (1 + 1j)
    return s


@pytest.mark.parametrize("lg", [15, 16, 17, 18, 19, 20])
@pytest.mark.parametrize("mode", [3, 4, 5])
def test_fourstep_bin_n2_carries_the_dc_term(mode, lg):
    """Modes 3, 4 and 5 do not patch bin n/2: it carries the offset-binary DC term, which fsea_fs_epilogue_kernel adds after
    the transform (`add_dc && k == n / 2`, interleaved with the `k -= 1` of the patched modes; 0.5f * (float)n, exact in f32
    up to 2^20).  A frame of zero bytes read as raw int8 has nothing else: 0.5 n (1 + i) in bin n/2, nothing in any other
    bin.  Modes 4 and 5 (the MAG_NODC and DB_F32 branches) never ran on this path; every (n1, n2) split."""
    n = 1 << lg
    want = dc_only_spectra(n)
    plan = fsea.Plan(n, mode=mode)
    got = exec_resident(plan, np.zeros(2 * n, np.uint8), 1)
    plan.close()
    if mode == 5:
        parity.check_db(got, parity.rows_of_spectra(want, 5), np.abs(want))
        # every other bin: below the peak by more than check_float's per-bin bound of 2e-6 of it (-114 dB)
        assert np.delete(got[0], n // 2).max() <= got[0, n // 2] - 100.0
    else:
        parity.check_spectra(got, want, mode)


def test_fourstep_float_input_resident_on_the_device():
    """in_f32 of fsea_fs_prep_kernel (8-byte samples: chunk and frame offsets in_bps = 8, no DC term: add_dc = 0) at 2^17
    points = 512 x 256.  The C ABI's float entry point is fsea_exec_f64_host; 3 frames of 2^17 f64 samples are more than its
    mapped-staging limit, so the doubles are narrowed on the device and the four-step launch reads f32 that is resident
    there (the 1 frame at 32768 of test_transform_sizes_above_the_largest_kernel reads mapped host memory).  The samples are
    f32 values, so the narrowing is exact and the f64 reference sees the numbers the kernel sees.  hop = n and an odd hop."""
    n, nf = 1 << 17, 3
    for hop, mode in ((n, 0), (n, 3), (4097, 3)):
        x = np.random.default_rng(17 + hop).normal(0, 0.3, 2 * ((nf - 1) * hop + n)).astype(np.float32).astype(np.float64)
        spectra = np.stack([np.fft.fft(O.unpack_center_f64(x[2 * f * hop: 2 * (f * hop + n)])) for f in range(nf)])
        plan = fsea.Plan(n, hop=hop, mode=mode)
        got = plan.exec_host_f64(x, nf)
        plan.close()
        parity.check_spectra(got, spectra, mode)
        check_patched_bin(got, n, mode)


# ---------------------------------------------------------------------------------------------
# 3. Bluestein sizes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5, 8, 31, 33])
def test_bluestein_smallest_sizes_and_the_neighbours_of_the_smallest_kernel(n):
    """3, 4, 5, 8: where `k == n / 2 && k > 0` of fsea_blu_epilogue_kernel patches bin 1, 2, 2 and 4 of rows this short and,
    for odd n, blu_setup's DC table 2 / (1 - r_k) puts the offset-binary term into every bin (m = 32, the smallest inner
    kernel, nearly all padding); 31 and 33: either side of the smallest size with a kernel (m = 64 and 128).  Modes 0-5
    (mode 5 never ran on this path), both byte conventions, hop = n and hop = 1, against the oracle's long-double DFT."""
    nf = 3
    for hop in (n, 1):
        iq = frames_iq(8000 + 10 * n + hop, n, nf, hop)
        spectra = parity.any_size_spectra(iq, n, nf, hop, True, exact=True)
        offset_binary = iq ^ FLIP_MASK
        for mode in range(6):
            plan = fsea.Plan(n, hop=hop, mode=mode)
            assert plan.kernel_name.startswith("bluestein(fsea_fft")
            for flip in (True, False):
                got = exec_resident(plan, iq if flip else offset_binary, nf, flip=flip)
                parity.check_spectra(got, spectra, mode)
                check_patched_bin(got, n, mode)
            plan.close()


@pytest.mark.parametrize("n,nf,inner", [(8193, 3, "bluestein(fourstep("), (16383, 3, "bluestein(fourstep("),
                                        (16385, 3, "bluestein(fourstep("), (524287, 1, "bluestein(fourstep(")])
def test_bluestein_on_fourstep_inner_transforms_up_to_the_largest_size(n, nf, inner):
    """8193: the first size whose inner transform (m = 32768) is a four-step plan; 16383 and 16385: either side of the largest
    kernel (16385 doubles m to 65536); 524287: the largest size bluestein_m takes, m = 2^20 on 1024 x 1024, chirp phases
    j^2 mod 2n up to 2^38 before the reduction, 8 frames per chunk.  Modes 0, 2, 3 and 5 (all four branches of the
    epilogue's output types), raw int8 bytes."""
    iq, spectra = case(n, nf, n, 9000 + n % 1000)
    for mode in (0, 2, 3, 5):
        plan = fsea.Plan(n, mode=mode)
        assert plan.kernel_name.startswith(inner)
        got = exec_resident(plan, iq, nf)
        plan.close()
        parity.check_spectra(got, spectra, mode)
        check_patched_bin(got, n, mode)


def check_edge_rows(got, spectra, centred, mode):
    """check_spectra, except where the reference row itself is numerically empty (below 1e-5 of the frame's largest spectral
    magnitude, the floor check_db has): a relative error against rounding noise or against exactly zero says nothing.
    Such a row is held to check_float's two bounds taken at the scale of what the f32 arithmetic carries -- the larger of
    the frame's whole spectrum and the spectrum of its centred samples (u - 128) / 256, which fsea_blu_prep_kernel
    transforms while the offset's spectrum comes from blu_setup's double table: per bin 2e-6 of the largest magnitude
    (+1e-6), in L2 1e-6 of the norm."""
    want = parity.rows_of_spectra(spectra, mode)
    if mode not in (0, 3):
        return parity.check_spectra(got, spectra, mode)
    full = max(np.abs(spectra).max(), np.abs(centred).max())
    if np.abs(want).max() > 1e-5 * full:
        return parity.check_float(got, want)
    err = np.abs(np.asarray(got, dtype=want.dtype) - want)
    norm = max(np.linalg.norm(spectra), np.linalg.norm(centred))
    print("empty reference row, mode %d: per-bin error %.3e (bound %.3e), L2 error %.3e (bound %.3e)" % (
        mode, err.max(), parity.PER_BIN_TOL * full + 1e-6, np.linalg.norm(err), parity.REL_L2_TOL * norm))
    assert err.max() <= parity.PER_BIN_TOL * full + 1e-6, "empty row: per-bin error %.3e > %.3e" % (
        err.max(), parity.PER_BIN_TOL * full + 1e-6)
    assert np.linalg.norm(err) <= parity.REL_L2_TOL * norm, "empty row: L2 error %.3e > %.3e" % (
        np.linalg.norm(err), parity.REL_L2_TOL * norm)


@pytest.mark.parametrize("n", [5, 1001, 8, 1000])
def test_bluestein_edge_inputs(n):
    """All-zero bytes, all-0xFF bytes and the alternating extremes of the emulation tier's test_edge_inputs, under both byte
    conventions.  Zero bytes read as raw int8 are the offset-binary constant alone: for odd n (5, 1001) every bin of the
    row is blu_setup's DC table and nothing else, for even n (8, 1000) one bin is -- and MAG rows patch that bin away, so
    the reference row is rounding noise of 1e-19 (the kernel's is exactly zero).  Read as offset binary they are negative
    full scale on both axes: the f32 transform of -0.5 (1 + i) and the table's +0.5 (1 + i) cancel to an exactly zero
    reference, which Bluestein's algorithm reaches to f32 rounding of the two parts (measured at 1001 points: 6.8e-5 per bin,
    2.1e-4 in L2 over two rows, the parts being 450 per bin and 1001 in L2; at 1000 points 1.1e-4 per bin; the sizes with
    kernels cancel exactly).  Rows like these
    two are compared by check_edge_rows' rule for an empty reference, every other row by check_float as it stands.
    Full-scale input is where the (u - 128) / 256 of fsea_blu_prep_kernel and the table have the least room."""
    nf = 2
    patterns = {"zero": np.zeros(2 * nf * n, np.uint8), "ones": np.full(2 * nf * n, 0xFF, np.uint8),
                "extremes": np.resize(np.array([0x7f, 0x80, 0x80, 0x7f], np.uint8), 2 * nf * n)}
    plans = {mode: fsea.Plan(n, mode=mode) for mode in (0, 2, 3, 5)}
    misses = []
    for flip in (True, False):
        # u8 128 in this byte convention: the offset alone
        offset = parity.any_size_spectra(np.full(2 * n, 0x00 if flip else 0x80, np.uint8), n, 1, n, flip, exact=True)
        for name, iq in patterns.items():
            spectra = parity.any_size_spectra(iq, n, nf, n, flip, exact=True)
            for mode, plan in plans.items():
                got = exec_resident(plan, iq, nf, flip=flip)
                try:
                    check_edge_rows(got, spectra, spectra - offset, mode)
                    check_patched_bin(got, n, mode)
                except AssertionError as e:
                    misses.append("%s flip=%s mode=%d: %s" % (name, flip, mode, str(e).splitlines()[0]))
    for plan in plans.values():
        plan.close()
    assert not misses, "\n".join(misses)


# ---------------------------------------------------------------------------------------------
# 4. no write outside the rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nf,mode", [(32768, 257, 1), (32768, 257, 3), (8191, 513, 1), (8191, 513, 3)])
def test_no_write_outside_the_rows_of_a_two_chunk_launch(n, nf, mode):
    """test_no_write_outside_the_output_rows of test_gpu_parity.py covers the sizes with kernels.  The any-size epilogues are
    grid-stride loops over nf * n elements behind a per-chunk base pointer: a chunk of 256 (512) frames then one of a single
    frame, rows of 1 byte (mode 1: a row of 8191 bytes ends at an odd address) and of 8 bytes (mode 3), 64 KiB of 0xA5 on
    either side of the rows -- exec_resident asserts both bands for every launch of this file -- and every row inside
    against the reference: an overrun, or a last chunk left short, shows."""
    iq, spectra = case(n, nf, n, 5000 + n % 1000 if is_fourstep(n) else 6000 + n % 1000)
    plan = fsea.Plan(n, mode=mode)
    got = exec_resident(plan, iq, nf)
    plan.close()
    parity.check_spectra(got, spectra, mode)


# ---------------------------------------------------------------------------------------------
# 5. shared work buffers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nf", [(1000, 1500), (32768, 200)])
def test_two_streams_and_two_threads_share_one_plans_work_buffers(n, nf):
    """A plan's two work buffers serve all its launches; launch() (fsea_plan.hip) orders them by work.ev / work.pending under
    work.mu.  Two launches of one plan back to back on two non-blocking streams, different inputs and outputs, nothing
    between them: without the wait the second launch's prep kernel overwrites buffer 0 under the first launch's transforms.
    Then the same from two host threads, three launches each.  Every row of both outputs against the reference (numpy's
    FFT at 1000 points too: 3000 rows).  One chunk each (1500 <= 4096, 200 <= 256): the seams have tests of their own.
    A probe for the race, not a proof of its absence: whether the second launch would overtake the first without the wait
    depends on the timing of the run, and the thread phase compares with the rows checked before."""
    assert nf <= work_frames(n)
    data = [case(n, nf, n, 11000 + k) for k in range(2)]
    plan = fsea.Plan(n)
    streams = [fsea.Stream(0), fsea.Stream(0)]
    d_in = [upload(DeviceBuffer(iq.nbytes), iq) for iq, _ in data]
    d_out = [DeviceBuffer(nf * plan.row_bytes) for _ in data]
    zeros = np.zeros(nf * n, np.float32)

    def rows(k):
        got = download(d_out[k], np.float32, (nf, n))
        upload(d_out[k], zeros)
        return got

    for k in range(2):
        plan.exec_device(d_in[k].ptr, nf, d_out[k].ptr, stream=streams[k])
    for k in range(2):
        plan.synchronize(streams[k])
    first = [rows(k) for k in range(2)]
    for k in range(2):
        parity.check_spectra(first[k], data[k][1], 0)

    errors = []

    def worker(k):
        try:
            for _ in range(3):
                plan.exec_device(d_in[k].ptr, nf, d_out[k].ptr, stream=streams[k])
                plan.synchronize(streams[k])
                if not np.array_equal(rows(k), first[k]):
                    raise AssertionError("thread %d: rows differ from the checked ones" % k)
        except Exception as e:          # noqa: BLE001 -- handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for b in d_in + d_out:
        b.free()
    plan.close()
    for s in streams:
        s.close()
    assert not errors, errors


# ---------------------------------------------------------------------------------------------
# 6. refusals stay refusals; the other entry points work
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,path", [(1000, "Bluestein's algorithm"), (32768, "the four-step decomposition")])
def test_entry_points_an_any_size_plan_refuses_and_those_it_serves(n, path):
    """launch() and fsea_plan_set_window refuse what the any-size paths do not have, with FSEA_EINVAL and a text that names
    the path: the frequency-shifted entry points (device and host; asserted before only for the device one on Bluestein,
    in test_transform_sizes_fftw_takes_and_the_kernels_do_not), the tiled entry point, a taper window.  A refusal leaves the
    plan usable: mean_magnitude_device (MAG_NODC rows into the plan's scratch, whatever the plan's mode), exec_host_into
    and reset then give the reference's numbers."""
    nf = 8 if n == 1000 else 2
    iq, spectra = case(n, nf, n, 12000 + n % 1000)
    plan = fsea.Plan(n, mode=fsea.MODE_DB10_U8)
    d_in = upload(DeviceBuffer(iq.nbytes), iq)
    d_out = DeviceBuffer(64 * n)
    with pytest.raises(fsea.FseaError, match=path):
        plan.exec_shifted_device(d_in.ptr, 1, d_out.ptr, 0.01)
    with pytest.raises(fsea.FseaError, match=path):
        plan.exec_shifted_host(iq, 1, 0.01)
    with pytest.raises(fsea.FseaError, match="the tiled entry points exist"):
        plan.exec_tiled_device(d_in.ptr, 64, d_out.ptr, 64, n, 0, 64, n)      # one tile of 64 rows: a valid geometry
    with pytest.raises(fsea.FseaError, match="no kernel of its own"):
        plan.set_window("hann")
    assert plan.window_form == 0
    mean = plan.mean_magnitude_device(d_in.ptr, nf)
    want = O.mean_magnitude(spectra)
    assert abs(mean - want) <= 2e-6 * want
    out = np.zeros((nf, n), np.uint8)
    plan.exec_host_into(iq, nf, out)
    parity.check_spectra(out, spectra, 1)
    plan.reset()
    assert np.array_equal(plan.exec_host(iq, nf), out)
    d_in.free()
    d_out.free()
    plan.close()


def test_fourstep_plan_refuses_a_capturing_stream():
    """fs_launch is five launches plus those of its inner plans through plan-owned buffers ordered by events: launch() refuses
    a stream that is being captured.  The Bluestein half of this is asserted in
    test_windowed_launches_capture_too_and_the_anysize_paths_refuse_a_capturing_stream (test_gpu_parity.py); the four-step
    branch of the message was not.  Nothing is enqueued by the refused call (the capture ends with an empty graph); before
    and after the capture the same call on the same stream gives the reference's rows."""
    hip = ctypes.CDLL("libamdhip64.so")
    n, nf = 32768, 2
    iq, spectra = case(n, nf, n, 12000 + n % 1000)
    plan = fsea.Plan(n)
    stream = fsea.Stream(0)
    d_in = upload(DeviceBuffer(iq.nbytes), iq)
    d_out = DeviceBuffer(nf * plan.row_bytes)

    def rows():
        plan.exec_device(d_in.ptr, nf, d_out.ptr, stream=stream)
        plan.synchronize(stream)
        got = download(d_out, np.float32, (nf, n))
        upload(d_out, np.zeros(nf * n, np.float32))
        return got

    parity.check_spectra(rows(), spectra, 0)
    graph = ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(stream.handle, 2) == 0            # hipStreamCaptureModeRelaxed
    try:
        with pytest.raises(fsea.FseaError, match="four-step decomposition, whose launches cannot be captured"):
            plan.exec_device(d_in.ptr, nf, d_out.ptr, stream=stream)
    finally:
        assert hip.hipStreamEndCapture(stream.handle, ctypes.byref(graph)) == 0
    if graph:
        hip.hipGraphDestroy(graph)
    parity.check_spectra(rows(), spectra, 0)
    d_in.free()
    d_out.free()
    plan.close()
    stream.close()
