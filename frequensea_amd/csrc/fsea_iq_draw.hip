// fsea_iq_draw.hip -- IQ constellation images (include/fsea.h: fsea_iq_*), the batched form of the reference's
// nrf_buffer_to_iq_points and nrf_buffer_to_iq_lines (src/nrf.c:359-421, 519-553).
//
// The coordinate of one element is the reference's nut_buffer_get_u8: a u8 element as is (optionally flipped), an f64 or
// f32 element v as x86-64's (uint8_t)(v * 256.0): cvttsd2si to int32 (0x80000000 for NaN and any truncation outside the
// int32 range), then the low byte.  AMDGPU's v_cvt_i32_f64 saturates instead, so the range check is explicit here.
//
// fsea_iq_points ("The IQ constellation images"): two workgroups of 1024 lanes per frame, each owning
// the half of the 256 x 256 bins with one value of I's top bit as a u32 histogram in 128 KiB of LDS.  Both read the whole
// frame.  Workgroups are dealt round-robin over the 8 XCDs, each with its own L2, so the two halves of a frame are blocks
// b and b + 8 (one XCD): in each group of 16 blocks, block b draws half (b >> 3) & 1 of frame 8 * (b >> 4) + (b & 7), and
// the second read of a frame can hit that XCD's L2.  The placement is a speed matter only; any placement gives the same
// image.  They count with ds_add_u32 and write the low byte of each count (the reference's wrapping u8++) as 16-byte
// stores.
//
// fsea_iq_lines: one lane per segment computes its endpoints and pixel count max(dx, dy) + 1; a wave-wide prefix sum then
// deals the wave's pixels out to its lanes 64 at a time, so a long segment is drawn by many lanes and the wave never waits
// on its longest segment.  Pixel t of a segment comes from the closed form of the reference's draw_line (fsea_iq_raster.h,
// shared with fsea_trace.hip; proved equal to the loop for every (dx, dy) in tests/test_iq_draw_host.py) and is counted with a u32 global atomic; a second
// kernel clamps the counts to 255 (the reference's saturating pixel_inc).
#include "fsea_internal.h"
#include "fsea_iq_raster.h"

#include <algorithm>
#include <cstring>

using fsea_detail::coord_f64;
using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int IQ_RES = 256;
constexpr int IQ_BINS = IQ_RES * IQ_RES;
constexpr int PTS_WG = 1024;
constexpr int PTS_HALF = IQ_BINS / 2;                 // bins per workgroup: u32 counts, 128 KiB of LDS
constexpr int PTS_CHUNK_FRAMES = 1 << 16;             // frames per points launch (2^17 workgroups, far below the grid limit)
constexpr int LN_WG = 256;
constexpr int CLAMP_WG = 256;
constexpr size_t LN_CHUNK_BYTES = (size_t)128 << 20;  // u32 counts of the frames one rasteriser launch draws
constexpr size_t MAX_ELEMS = (size_t)1 << 40;

template <int T> struct PairBytes;
template <> struct PairBytes<FSEA_IQ_U8> { static constexpr int v = 2; };
template <> struct PairBytes<FSEA_IQ_F32> { static constexpr int v = 8; };
template <> struct PairBytes<FSEA_IQ_F64> { static constexpr int v = 16; };

// pair k of the input: (I, Q) coordinates in [0, 255]
template <int T>
__device__ __forceinline__ void load_pair(const void *__restrict__ in, long long k, uint32_t flip, uint32_t &I, uint32_t &Q) {
    if (T == FSEA_IQ_U8) {
        const uint32_t b = ((uint32_t)(static_cast<const uint16_t *>(in))[k] ^ flip) & 0xffffu;
        I = b & 0xffu;
        Q = b >> 8;
    } else if (T == FSEA_IQ_F32) {
        const float2 f = (static_cast<const float2 *>(in))[k];
        I = coord_f64((double)f.x);
        Q = coord_f64((double)f.y);
    } else {
        const double2 d = (static_cast<const double2 *>(in))[k];
        I = coord_f64(d.x);
        Q = coord_f64(d.y);
    }
}

// the 16 / PairBytes pairs of one aligned 16-byte group
template <int T>
__device__ __forceinline__ void decode_group(uint4 q, uint32_t flip, uint32_t *I, uint32_t *Q) {
    if (T == FSEA_IQ_U8) {
        const uint32_t w[4] = {q.x ^ flip, q.y ^ flip, q.z ^ flip, q.w ^ flip};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            I[2 * j] = w[j] & 0xffu;
            Q[2 * j] = (w[j] >> 8) & 0xffu;
            I[2 * j + 1] = (w[j] >> 16) & 0xffu;
            Q[2 * j + 1] = w[j] >> 24;
        }
    } else if (T == FSEA_IQ_F32) {
        I[0] = coord_f64((double)__uint_as_float(q.x));
        Q[0] = coord_f64((double)__uint_as_float(q.y));
        I[1] = coord_f64((double)__uint_as_float(q.z));
        Q[1] = coord_f64((double)__uint_as_float(q.w));
    } else {
        I[0] = coord_f64(__hiloint2double((int)q.y, (int)q.x));
        Q[0] = coord_f64(__hiloint2double((int)q.w, (int)q.z));
    }
}

template <int T>
__device__ __forceinline__ void points_body(const void *__restrict__ in, long long n_pairs, uint32_t flip,
                                            long long frame0, int n_frames, uint8_t *__restrict__ out) {
    constexpr int PB = PairBytes<T>::v;
    constexpr int PPG = 16 / PB;  // pairs per 16-byte group
    __shared__ __attribute__((aligned(16))) uint32_t hist[PTS_HALF];
    const int tid = threadIdx.x;
    // the two halves of a frame 8 blocks apart, on one XCD; the last group of 16 blocks may run past the launch's frames
    const uint32_t b = blockIdx.x;
    const int local = (int)(b >> 4) * 8 + (int)(b & 7);
    if (local >= n_frames) return;
    const long long frame = frame0 + local;
    const uint32_t half = (b >> 3) & 1u;
    for (int i = tid; i < PTS_HALF / 4; i += PTS_WG) reinterpret_cast<uint4 *>(hist)[i] = uint4{0u, 0u, 0u, 0u};
    __syncthreads();

    // the frame's bytes [b0, b1) in aligned 16-byte groups; only the first and the last group can be partial, and those
    // are read pair by pair (the last may end past the input)
    const long long b0 = frame * n_pairs * PB, b1 = b0 + n_pairs * PB;
    const long long g1 = (b1 + 15) >> 4;
    for (long long g = (b0 >> 4) + tid; g < g1; g += PTS_WG) {
        uint32_t I[PPG], Q[PPG];
        bool ok[PPG];
        if (16 * g >= b0 && 16 * g + 16 <= b1) {
            decode_group<T>((static_cast<const uint4 *>(in))[g], flip, I, Q);
#pragma unroll
            for (int j = 0; j < PPG; ++j) ok[j] = true;
        } else {
#pragma unroll
            for (int j = 0; j < PPG; ++j) {
                const long long b = 16 * g + j * PB;
                ok[j] = b >= b0 && b < b1;
                I[j] = Q[j] = 0u;
                if (ok[j]) load_pair<T>(in, b / PB, flip, I[j], Q[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < PPG; ++j) {
            if (ok[j] && (I[j] >> 7) == half) atomicAdd(&hist[((I[j] & 127u) << 8) | Q[j]], 1u);
        }
    }
    __syncthreads();

    // the low byte of each count (the reference's u8++ wraps), 16 bins per 16-byte store
    uint4 *o = reinterpret_cast<uint4 *>(out + frame * IQ_BINS + (long long)half * PTS_HALF);
    for (int i = tid; i < PTS_HALF / 16; i += PTS_WG) {
        const uint4 *h = reinterpret_cast<const uint4 *>(hist) + 4 * i;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4 c = h[j];
            w[j] = (c.x & 0xffu) | (c.y & 0xffu) << 8 | (c.z & 0xffu) << 16 | (c.w & 0xffu) << 24;
        }
        o[i] = uint4{w[0], w[1], w[2], w[3]};
    }
}

// grid (ceil(segments / LN_WG), frames of this launch); counts: one (256 m)^2 u32 image per frame of the launch
template <int T>
__device__ __forceinline__ void lines_body(const void *__restrict__ in, long long n_points, uint32_t flip, int m,
                                           long long frame0, uint32_t *__restrict__ counts) {
    const uint32_t stride = (uint32_t)(IQ_RES * m);
    const long long frame = frame0 + blockIdx.y;
    uint32_t *img = counts + (size_t)blockIdx.y * stride * stride;
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * LN_WG + threadIdx.x;  // segment s: point s to point s + 1

    uint32_t A = 0u, B = 0u, len = 0u;
    if (s + 1 < n_points) {
        uint32_t I1, Q1, I2, Q2;
        load_pair<T>(in, frame * n_points + s, flip, I1, Q1);
        load_pair<T>(in, frame * n_points + s + 1, flip, I2, Q2);
        A = I1 * m | (Q1 * m) << 16;
        B = I2 * m | (Q2 * m) << 16;
        const int dx = abs((int)(I2 - I1)) * m, dy = abs((int)(Q2 - Q1)) * m;
        len = (uint32_t)max(dx, dy) + 1u;
    }
    // every lane stays active through the deal of the wave's pixels (fsea_iq_raster.h); only the atomic is predicated
    fsea_detail::wave_lines(A, B, len, lane, [&](uint32_t sA, uint32_t sB, uint32_t t) {
        atomicAdd(img + fsea_detail::line_pixel(sA, sB, t, stride), 1u);
    });
}

}  // namespace

extern "C" __global__ __launch_bounds__(PTS_WG) void fsea_iq_points_u8(const void *__restrict__ in, long long n_pairs,
                                                                    uint32_t flip, long long frame0, int n_frames,
                                                                    uint8_t *__restrict__ out) {
    points_body<FSEA_IQ_U8>(in, n_pairs, flip, frame0, n_frames, out);
}
extern "C" __global__ __launch_bounds__(PTS_WG) void fsea_iq_points_f32(const void *__restrict__ in, long long n_pairs,
                                                                    uint32_t flip, long long frame0, int n_frames,
                                                                    uint8_t *__restrict__ out) {
    points_body<FSEA_IQ_F32>(in, n_pairs, flip, frame0, n_frames, out);
}
extern "C" __global__ __launch_bounds__(PTS_WG) void fsea_iq_points_f64(const void *__restrict__ in, long long n_pairs,
                                                                    uint32_t flip, long long frame0, int n_frames,
                                                                    uint8_t *__restrict__ out) {
    points_body<FSEA_IQ_F64>(in, n_pairs, flip, frame0, n_frames, out);
}

extern "C" __global__ __launch_bounds__(LN_WG) void fsea_iq_lines_u8(const void *__restrict__ in, long long n_points,
                                                                      uint32_t flip, int m, long long frame0,
                                                                      uint32_t *__restrict__ counts) {
    lines_body<FSEA_IQ_U8>(in, n_points, flip, m, frame0, counts);
}
extern "C" __global__ __launch_bounds__(LN_WG) void fsea_iq_lines_f32(const void *__restrict__ in, long long n_points,
                                                                       uint32_t flip, int m, long long frame0,
                                                                       uint32_t *__restrict__ counts) {
    lines_body<FSEA_IQ_F32>(in, n_points, flip, m, frame0, counts);
}
extern "C" __global__ __launch_bounds__(LN_WG) void fsea_iq_lines_f64(const void *__restrict__ in, long long n_points,
                                                                       uint32_t flip, int m, long long frame0,
                                                                       uint32_t *__restrict__ counts) {
    lines_body<FSEA_IQ_F64>(in, n_points, flip, m, frame0, counts);
}

// min(count, 255) for n16 groups of 16 pixels
extern "C" __global__ __launch_bounds__(CLAMP_WG) void fsea_iq_clamp(const uint4 *__restrict__ counts, long long n16,
                                                                     uint4 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * CLAMP_WG + threadIdx.x;
    if (i >= n16) return;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint4 c = counts[4 * i + j];
        w[j] = min(c.x, 255u) | min(c.y, 255u) << 8 | min(c.z, 255u) << 16 | min(c.w, 255u) << 24;
    }
    out[i] = uint4{w[0], w[1], w[2], w[3]};
}

struct fsea_iq_draw {
    int device = 0;
    std::mutex mu;
    fsea_detail::SharedScratch counts;  // u32 counts of the frames one rasteriser launch draws
    fsea_detail::HostStaging staging;   // the host-buffer forms
};

namespace {

size_t pair_bytes(int type) { return type == FSEA_IQ_U8 ? 2 : type == FSEA_IQ_F32 ? 8 : 16; }

int check_common(const fsea_iq_draw *d, int type, size_t n, int n_frames) {
    if (!d) return fail(FSEA_EINVAL, "iq_draw is NULL");
    if (type != FSEA_IQ_U8 && type != FSEA_IQ_F32 && type != FSEA_IQ_F64) return fail(FSEA_EINVAL, "unknown input type %d", type);
    if (int rc = fsea_detail::check_n_frames(n_frames)) return rc;
    if (n > ((size_t)1 << 31) || (n_frames && n > MAX_ELEMS / (size_t)n_frames)) {
        return fail(FSEA_EINVAL, "%zu pairs x %d frames is too large", n, n_frames);
    }
    return FSEA_OK;
}

// the caller holds d->mu and is on d's device
int points_launch(fsea_iq_draw *d, const void *d_iq, int type, int flip, size_t n_pairs, int n_frames, void *d_image,
                  hipStream_t s) {
    if (n_frames == 0) return FSEA_OK;
    if (n_pairs == 0) {
        FSEA_HIP(hipMemsetAsync(d_image, 0, (size_t)n_frames * IQ_BINS, s));
        return FSEA_OK;
    }
    const uint32_t fm = (type == FSEA_IQ_U8 && flip) ? 0x80808080u : 0u;
    const long long n = (long long)n_pairs;
    uint8_t *out = static_cast<uint8_t *>(d_image);
    for (int f0 = 0; f0 < n_frames; f0 += PTS_CHUNK_FRAMES) {
        const int nf = std::min(PTS_CHUNK_FRAMES, n_frames - f0);
        const dim3 grid(16u * (unsigned)((nf + 7) / 8));  // groups of 8 frames x 2 halves
        const long long fr = f0;
        if (type == FSEA_IQ_U8) {
            hipLaunchKernelGGL(fsea_iq_points_u8, grid, dim3(PTS_WG), 0, s, d_iq, n, fm, fr, nf, out);
        } else if (type == FSEA_IQ_F32) {
            hipLaunchKernelGGL(fsea_iq_points_f32, grid, dim3(PTS_WG), 0, s, d_iq, n, fm, fr, nf, out);
        } else {
            hipLaunchKernelGGL(fsea_iq_points_f64, grid, dim3(PTS_WG), 0, s, d_iq, n, fm, fr, nf, out);
        }
        FSEA_HIP(hipGetLastError());
    }
    return FSEA_OK;
}

int lines_launch(fsea_iq_draw *d, const void *d_iq, int type, int flip, size_t n_points, int n_frames, int m,
                 void *d_image, hipStream_t s) {
    if (n_frames == 0) return FSEA_OK;
    const size_t pixels = (size_t)IQ_RES * m * IQ_RES * m;
    if (n_points < 2) {
        FSEA_HIP(hipMemsetAsync(d_image, 0, (size_t)n_frames * pixels, s));
        return FSEA_OK;
    }
    const size_t chunk = std::min<size_t>((size_t)n_frames, std::max<size_t>(1, LN_CHUNK_BYTES / (4 * pixels)));
    // every use of the count buffer, on whatever stream, follows the previous one
    if (int rc = d->counts.acquire(chunk * pixels * 4, s)) return rc;
    uint32_t *d_counts = static_cast<uint32_t *>(d->counts.buf.ptr);
    const uint32_t fm = (type == FSEA_IQ_U8 && flip) ? 0x80808080u : 0u;
    const long long n = (long long)n_points;
    const unsigned gx = (unsigned)((n_points - 1 + LN_WG - 1) / LN_WG);
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += chunk) {
        const size_t nf = std::min(chunk, (size_t)n_frames - f0);
        FSEA_HIP(hipMemsetAsync(d_counts, 0, nf * pixels * 4, s));
        const dim3 grid(gx, (unsigned)nf);
        const long long fr = (long long)f0;
        if (type == FSEA_IQ_U8) {
            hipLaunchKernelGGL(fsea_iq_lines_u8, grid, dim3(LN_WG), 0, s, d_iq, n, fm, m, fr, d_counts);
        } else if (type == FSEA_IQ_F32) {
            hipLaunchKernelGGL(fsea_iq_lines_f32, grid, dim3(LN_WG), 0, s, d_iq, n, fm, m, fr, d_counts);
        } else {
            hipLaunchKernelGGL(fsea_iq_lines_f64, grid, dim3(LN_WG), 0, s, d_iq, n, fm, m, fr, d_counts);
        }
        FSEA_HIP(hipGetLastError());
        const long long n16 = (long long)(nf * pixels / 16);
        hipLaunchKernelGGL(fsea_iq_clamp, dim3((unsigned)((n16 + CLAMP_WG - 1) / CLAMP_WG)), dim3(CLAMP_WG), 0, s,
                           reinterpret_cast<const uint4 *>(d_counts), n16,
                           reinterpret_cast<uint4 *>(static_cast<uint8_t *>(d_image) + f0 * pixels));
        FSEA_HIP(hipGetLastError());
    }
    return d->counts.release(s);
}

// the host-buffer forms: the launches through the object's staging (fsea_detail::HostStaging)
int draw_host(fsea_iq_draw *d, bool lines, const void *iq, int type, int flip, size_t n, int m, uint8_t *image) {
    const size_t pixels = (size_t)IQ_RES * m * IQ_RES * m;
    const size_t in_bytes = n * pair_bytes(type);
    std::lock_guard<std::mutex> lock(d->mu);
    FSEA_ON_DEVICE(d->device);
    return d->staging.run(
        in_bytes, pixels, image, [&](void *h_in) { std::memcpy(h_in, iq, in_bytes); },
        [&](void *d_in, void *d_out, hipStream_t s) {
            return lines ? lines_launch(d, d_in, type, flip, n, 1, m, d_out, s)
                         : points_launch(d, d_in, type, flip, n, 1, d_out, s);
        });
}

}  // namespace

extern "C" {

int fsea_iq_draw_create(fsea_iq_draw **out, int device) {
    if (!out) return fail(FSEA_EINVAL, "iq_draw out-pointer is NULL");
    *out = nullptr;
    return fsea_detail::create_object(out, device, "fsea_iq_draw_create",
                                      [](fsea_iq_draw *d) { return d->counts.create(d->staging.stream); });
}

int fsea_iq_draw_destroy(fsea_iq_draw *d) { return fsea_detail::destroy_object(d); }

int fsea_iq_points_device(fsea_iq_draw *d, const void *d_iq, int type, int flip, size_t n_pairs, int n_frames,
                          void *d_image, void *stream) {
    int rc = check_common(d, type, n_pairs, n_frames);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    if ((n_pairs && !d_iq) || !d_image) return fail(FSEA_EINVAL, "NULL buffer");
    rc = fsea_detail::check_aligned16("d_iq and d_image", d_iq, d_image);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(d->mu);
    FSEA_ON_DEVICE(d->device);
    return points_launch(d, d_iq, type, flip, n_pairs, n_frames, d_image, static_cast<hipStream_t>(stream));
}

int fsea_iq_lines_device(fsea_iq_draw *d, const void *d_iq, int type, int flip, size_t n_points, int n_frames,
                         int size_multiplier, void *d_image, void *stream) {
    int rc = check_common(d, type, n_points, n_frames);
    if (!rc) rc = fsea_detail::check_multiplier(size_multiplier);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    if ((n_points && !d_iq) || !d_image) return fail(FSEA_EINVAL, "NULL buffer");
    rc = fsea_detail::check_aligned16("d_iq and d_image", d_iq, d_image);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(d->mu);
    FSEA_ON_DEVICE(d->device);
    return lines_launch(d, d_iq, type, flip, n_points, n_frames, size_multiplier, d_image, static_cast<hipStream_t>(stream));
}

int fsea_iq_points_host(fsea_iq_draw *d, const void *iq, int type, int flip, size_t n_pairs, uint8_t *image) {
    int rc = check_common(d, type, n_pairs, 1);
    if (rc) return rc;
    if ((n_pairs && !iq) || !image) return fail(FSEA_EINVAL, "NULL buffer");
    return draw_host(d, false, iq, type, flip, n_pairs, 1, image);
}

int fsea_iq_lines_host(fsea_iq_draw *d, const void *iq, int type, int flip, size_t n_points, int size_multiplier,
                       uint8_t *image) {
    int rc = check_common(d, type, n_points, 1);
    if (!rc) rc = fsea_detail::check_multiplier(size_multiplier);
    if (rc) return rc;
    if ((n_points && !iq) || !image) return fail(FSEA_EINVAL, "NULL buffer");
    return draw_host(d, true, iq, type, flip, n_points, size_multiplier, image);
}

}  // extern "C"
