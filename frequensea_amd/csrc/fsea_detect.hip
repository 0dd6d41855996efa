// fsea_detect.hip -- the burst detector of the reference's signal scene (include/fsea.h: fsea_detect_*): the statistics of
// nrf_signal_detector_process (src/nrf.c:883-898) for many sample blocks per launch.
//
// The device computes three exact integer sums per block of 8-bit samples -- the bytes at even offsets, all bytes, all
// squares -- and the host turns them into the reference's mean and standard deviation (fsea_detect_moments, below).  The
// kernels are a pure read stream: 16-byte loads per lane, four in flight, and three v_dot4_u32_u8 per dword (multipliers
// 0x00010001, 0x01010101 and the dword itself).  A lane sums in 32 bits: a dword adds at most 4 * 255^2 = 260100 to the
// squares, so 16512 dwords fit, and the host never gives a lane more than DT_MAX_LANE_DWORDS = 16384 of them before its
// sums are widened to 64 bits for the reduction (across the wave by shuffles, across the waves of a workgroup through LDS).
// Integer sums have one value whatever the order: the result does not depend on the grid.
//
// Two kernels, chosen by the block size ("The burst detector"):
//   fsea_detect_waves   blocks of at most DT_WAVE_BLOCK bytes: one wave per block, the waves striding over the blocks;
//                       lane 0 stores the three sums.  No LDS, no barrier, no atomic.
//   fsea_detect_slices  larger blocks: one workgroup per slice of a block.  With one slice per block thread 0 stores the
//                       sums; with several it adds them with 64-bit atomics to sums that the launch zeroed before.
// A block starts at a multiple of 2 bytes only, so a range [a, b) of the buffer is summed in three parts: the bytes in
// front of the first 16-byte boundary and those behind the last one by one lane each, what lies between by aligned loads.
// Nothing outside [a, b) is read.  The buffer's base is 16-byte aligned and a block's size is even: a byte's offset in its
// block is even exactly when its offset in the buffer is, which is what picks the bytes of the first sum.
#include "fsea_internal.h"

#include <algorithm>
#include <cmath>
#include <memory>

using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int DT_WG = 256;
constexpr size_t DT_WAVE_BLOCK = 16384;          // largest block one wave takes whole
constexpr size_t DT_MIN_SLICE = 16384;           // one round of a workgroup: 256 lanes x 4 loads x 16 bytes
constexpr size_t DT_MAX_LANE_DWORDS = 16384;     // 32-bit lane sums hold 16512 dwords of squares
constexpr size_t DT_MAX_SLICE = DT_MAX_LANE_DWORDS * 4 * DT_WG;   // 16 MiB: what keeps a lane of a workgroup within it
constexpr size_t DT_MAX_BLOCK = (size_t)1 << 31;  // elements per block, as the reference's int
constexpr size_t DT_MAX_TOTAL = (size_t)1 << 40;
static_assert(DT_WAVE_BLOCK / 4 / 64 <= DT_MAX_LANE_DWORDS, "a wave's lane stays within its 32-bit sums");

struct Sums {
    uint32_t even, all, squares;
};

__device__ __forceinline__ void add_dword(Sums &s, uint32_t w, uint32_t flip) {
    w ^= flip;
    s.even = __builtin_amdgcn_udot4(w, 0x00010001u, s.even, false);
    s.all = __builtin_amdgcn_udot4(w, 0x01010101u, s.all, false);
    s.squares = __builtin_amdgcn_udot4(w, w, s.squares, false);
}

__device__ __forceinline__ void add_vector(Sums &s, const uint4 &v, uint32_t flip) {
    add_dword(s, v.x, flip);
    add_dword(s, v.y, flip);
    add_dword(s, v.z, flip);
    add_dword(s, v.w, flip);
}

__device__ __forceinline__ void add_byte(Sums &s, const uint8_t *__restrict__ base, size_t at, uint32_t flip) {
    const uint32_t v = (uint32_t)base[at] ^ (flip & 0xffu);
    if (!(at & 1)) s.even += v;
    s.all += v;
    s.squares += v * v;
}

// The sums of the bytes [a, b) of the buffer as lane t of a group of G lanes sees them; the group's lanes together cover
// the range once.
template <int G>
__device__ __forceinline__ Sums range_sums(const uint8_t *__restrict__ base, size_t a, size_t b, int t, uint32_t flip) {
    Sums s = {0u, 0u, 0u};
    const size_t a16 = (a + 15) & ~(size_t)15, b16 = b & ~(size_t)15;
    const size_t head_end = a16 < b ? a16 : b;       // [a, head_end): in front of the first boundary
    const size_t tail = a16 > b16 ? a16 : b16;       // [tail, b): behind the last one
    if (a + (size_t)t < head_end) add_byte(s, base, a + (size_t)t, flip);
    if (tail + (size_t)t < b) add_byte(s, base, tail + (size_t)t, flip);
    if (a16 < b16) {
        const uint4 *__restrict__ p = reinterpret_cast<const uint4 *>(base + a16);
        const size_t n = (b16 - a16) / 16;
        size_t i = (size_t)t;
        for (; i + 3 * G < n; i += 4 * G) {
            const uint4 v0 = p[i], v1 = p[i + G], v2 = p[i + 2 * G], v3 = p[i + 3 * G];
            add_vector(s, v0, flip);
            add_vector(s, v1, flip);
            add_vector(s, v2, flip);
            add_vector(s, v3, flip);
        }
        for (; i < n; i += G) add_vector(s, p[i], flip);
    }
    return s;
}

// the sum over the wave's lanes, in lane 0
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

}  // namespace

// grid: any number of workgroups of DT_WG threads; sums: three u64 per block
extern "C" __global__ __launch_bounds__(DT_WG) void fsea_detect_waves(const uint8_t *__restrict__ base, size_t block_bytes,
                                                                      size_t n_blocks, uint32_t flip,
                                                                      unsigned long long *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (DT_WG / 64);
    for (size_t b = (size_t)blockIdx.x * (DT_WG / 64) + (threadIdx.x >> 6); b < n_blocks; b += waves) {
        const Sums s = range_sums<64>(base, b * block_bytes, (b + 1) * block_bytes, lane, flip);
        const unsigned long long even = wave_sum(s.even), all = wave_sum(s.all), squares = wave_sum(s.squares);
        if (lane == 0) {
            sums[3 * b] = even;
            sums[3 * b + 1] = all;
            sums[3 * b + 2] = squares;
        }
    }
}

// grid: n_blocks * slices workgroups; workgroup u takes slice u % slices of block u / slices, slice_bytes (a multiple of
// 16) each but the last of a block.  slices > 1: sums are zero before the launch.
extern "C" __global__ __launch_bounds__(DT_WG) void fsea_detect_slices(const uint8_t *__restrict__ base, size_t block_bytes,
                                                                       uint32_t slices, size_t slice_bytes, uint32_t flip,
                                                                       unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long part[DT_WG / 64][3];
    const size_t b = blockIdx.x / slices, slice = blockIdx.x % slices;
    const size_t first = b * block_bytes, a = first + slice * slice_bytes;
    const size_t end = a + slice_bytes < first + block_bytes ? a + slice_bytes : first + block_bytes;
    const Sums s = range_sums<DT_WG>(base, a, end, (int)threadIdx.x, flip);
    const unsigned long long even = wave_sum(s.even), all = wave_sum(s.all), squares = wave_sum(s.squares);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = even;
        part[threadIdx.x >> 6][1] = all;
        part[threadIdx.x >> 6][2] = squares;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < DT_WG / 64; ++w) v += part[w][threadIdx.x];
        if (slices == 1) sums[3 * b + threadIdx.x] = v;
        else atomicAdd(sums + 3 * b + threadIdx.x, v);
    }
}

struct fsea_detect {
    int device = 0;
    unsigned target_wg = 2048;          // workgroups that occupy the card: 8 per CU
    std::mutex mu;
    fsea_detail::HostStaging staging;   // the host form
};

namespace {

// what does not look at the object comes first: a test can pass an object that is never dereferenced
int check_blocks(const fsea_detect *d, const void *iq, size_t block_bytes, size_t n_blocks) {
    if (!d) return fail(FSEA_EINVAL, "detect is NULL");
    if (block_bytes < 2 || (block_bytes & 1) || block_bytes > DT_MAX_BLOCK) {
        return fail(FSEA_EINVAL, "block_bytes must be even and in [2, 2^31], got %zu", block_bytes);
    }
    if (n_blocks == 0 || n_blocks > DT_MAX_TOTAL / block_bytes) {
        return fail(FSEA_EINVAL, "n_blocks must be at least 1 and the blocks at most 2^40 bytes, got %zu x %zu", n_blocks,
                    block_bytes);
    }
    if (!iq) return fail(FSEA_EINVAL, "NULL buffer");
    return FSEA_OK;
}

// the caller is on d's device
int detect_launch(const fsea_detect *d, const uint8_t *d_iq, size_t block_bytes, size_t n_blocks, int flip,
                  unsigned long long *d_sums, hipStream_t s) {
    const uint32_t fm = flip ? 0x80808080u : 0u;
    if (block_bytes <= DT_WAVE_BLOCK) {
        const size_t wgs = std::min<size_t>((n_blocks + DT_WG / 64 - 1) / (DT_WG / 64), d->target_wg);
        hipLaunchKernelGGL(fsea_detect_waves, dim3((unsigned)wgs), dim3(DT_WG), 0, s, d_iq, block_bytes, n_blocks, fm, d_sums);
        FSEA_HIP(hipGetLastError());
        return FSEA_OK;
    }
    // Slices per block: enough workgroups for the card while a slice stays a full round of loads, and never a slice that
    // would take a lane past its 32-bit sums.
    size_t slices = std::min((d->target_wg + n_blocks - 1) / n_blocks, (block_bytes + DT_MIN_SLICE - 1) / DT_MIN_SLICE);
    slices = std::max(slices, (block_bytes + DT_MAX_SLICE - 1) / DT_MAX_SLICE);
    const size_t slice_bytes = ((block_bytes + slices - 1) / slices + 15) & ~(size_t)15;
    slices = (block_bytes + slice_bytes - 1) / slice_bytes;
    if (slice_bytes > DT_MAX_SLICE || n_blocks * slices > 0x7fffffffu) {
        return fail(FSEA_EINVAL, "%zu blocks of %zu bytes are too many for one launch", n_blocks, block_bytes);
    }
    if (slices > 1) FSEA_HIP(hipMemsetAsync(d_sums, 0, 24 * n_blocks, s));
    hipLaunchKernelGGL(fsea_detect_slices, dim3((unsigned)(n_blocks * slices)), dim3(DT_WG), 0, s, d_iq, block_bytes,
                       (uint32_t)slices, slice_bytes, fm, d_sums);
    FSEA_HIP(hipGetLastError());
    return FSEA_OK;
}

}  // namespace

extern "C" {

int fsea_detect_create(fsea_detect **out, int device) {
    if (!out) return fail(FSEA_EINVAL, "detect out-pointer is NULL");
    *out = nullptr;
    return fsea_detail::create_object(out, device, "fsea_detect_create", [&](fsea_detect *d) {
        int cus = 0;
        hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        if (e == hipSuccess && cus > 0) d->target_wg = 8u * (unsigned)cus;
        return e;
    });
}

int fsea_detect_destroy(fsea_detect *d) { return fsea_detail::destroy_object(d); }

int fsea_detect_u8_device(fsea_detect *d, const void *d_iq, size_t block_bytes, size_t n_blocks, int flip, uint64_t *d_sums,
                          void *stream) {
    int rc = check_blocks(d, d_iq, block_bytes, n_blocks);
    if (rc) return rc;
    if (!d_sums) return fail(FSEA_EINVAL, "NULL buffer");
    rc = fsea_detail::check_aligned16("d_iq and d_sums", d_iq, d_sums);
    if (rc) return rc;
    FSEA_ON_DEVICE(d->device);
    return detect_launch(d, static_cast<const uint8_t *>(d_iq), block_bytes, n_blocks, flip,
                         reinterpret_cast<unsigned long long *>(d_sums), static_cast<hipStream_t>(stream));
}

int fsea_detect_u8_host(fsea_detect *d, const uint8_t *iq, size_t block_bytes, size_t n_blocks, int flip, double *mean,
                        double *sd) {
    int rc = check_blocks(d, iq, block_bytes, n_blocks);
    if (rc) return rc;
    if (!mean || !sd) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(d->mu);
    FSEA_ON_DEVICE(d->device);
    const size_t in_bytes = block_bytes * n_blocks;
    std::unique_ptr<uint64_t[]> sums(new (std::nothrow) uint64_t[3 * n_blocks]);
    if (!sums) return fail(FSEA_ENOMEM, "out of host memory");
    rc = d->staging.run(
        in_bytes, 24 * n_blocks, sums.get(), [&](void *h_in) { std::memcpy(h_in, iq, in_bytes); },
        [&](void *d_in, void *d_out, hipStream_t s) {
            return detect_launch(d, static_cast<const uint8_t *>(d_in), block_bytes, n_blocks, flip,
                                 static_cast<unsigned long long *>(d_out), s);
        });
    if (rc) return rc;
    for (size_t b = 0; b < n_blocks; ++b) {
        rc = fsea_detect_finish(sums.get() + 3 * b, block_bytes, mean + b, sd + b);
        if (rc) return rc;
    }
    return FSEA_OK;
}

// Host arithmetic; no device is touched.  With x_i = byte_i / 256: mean is the reference's own value bit for bit (its sum
// of the even elements is a sum of multiples of 1/256 below 2^53, exact in any order).  The sum of (x_i - mean)^2 is
// (S2 - 2 M S1 + n M^2) / 65536 with M = 256 mean, which cancels badly in double for a quiet block; so the sums are first
// centred on the integer c nearest to M, exactly in 64-bit integers (S2 < 2^47, n c^2 < 2^47, 2 c S1 < 2^48), and only the
// small remainder d = M - c, |d| <= 1/2, enters in double.
int fsea_detect_moments(const uint64_t sums[3], size_t n_elements, double *mean, double *diffs_total) {
    if (!sums || !mean || !diffs_total) return fail(FSEA_EINVAL, "NULL buffer");
    if (n_elements < 2 || (n_elements & 1) || n_elements > DT_MAX_BLOCK) {
        return fail(FSEA_EINVAL, "n_elements must be even and in [2, 2^31], got %zu", n_elements);
    }
    const uint64_t n = n_elements;
    if (sums[0] > 255 * (n / 2) || sums[1] > 255 * n || sums[2] > 65025 * n) {
        return fail(FSEA_EINVAL, "the sums are not those of %zu bytes", n_elements);
    }
    const double m = ((double)sums[0] / 256.0) / (double)n * 2;
    const double scaled = 256.0 * m;                       // exact: a power of two
    const int64_t c = (int64_t)std::llround(scaled);       // in [0, 255]
    const double d = scaled - (double)c;
    const int64_t s1c = (int64_t)sums[1] - (int64_t)n * c;
    const int64_t s2c = (int64_t)sums[2] - 2 * c * (int64_t)sums[1] + (int64_t)n * c * c;
    *mean = m;
    *diffs_total = ((double)s2c - 2.0 * d * (double)s1c + (double)n * d * d) / 65536.0;
    return FSEA_OK;
}

int fsea_detect_finish(const uint64_t sums[3], size_t n_elements, double *mean, double *sd) {
    if (!sd) return fail(FSEA_EINVAL, "NULL buffer");
    double diffs_total = 0.0;
    int rc = fsea_detect_moments(sums, n_elements, mean, &diffs_total);
    if (rc) return rc;
    *sd = std::sqrt(diffs_total / *mean);   // the reference divides by the mean, not by the count; 0 / 0 is its NaN too
    return FSEA_OK;
}

}  // extern "C"
