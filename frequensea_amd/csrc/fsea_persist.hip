// fsea_persist.hip -- the persistence spectrum (include/fsea.h: fsea_persist_*): counts[l * width + k], how often column k
// of the rows offered so far was at level l, the frequency-domain twin of the IQ constellation image (fsea_iq_draw.hip).
// Integer and order-free: every count is the same whatever the launch geometry or the cut of the rows into calls.
//
// Kernels fsea_persist_u8 / fsea_persist_f32 (and their _narrow forms; DESIGN.md section 4, "The persistence spectrum"): a
// workgroup of 256 lanes owns a tile of PS_C = 64 columns and a run of FSEA_PERSIST_RUN_ROWS rows, counts them into a
// 256 x 64 u32 histogram in 64 KiB of LDS (ds_add_u32; u32 counters, so no run can overflow one) and then adds the
// non-zero counters to the resident counts with u32 global atomics.  The grid is runs x column tiles.
//
// The histogram's row of a level holds the tile's columns in a permuted order: column c = 16 l + 4 k + j (digits base 4)
// sits at position rev(c) = 16 j + 4 k + l, an involution.  The LDS bank of a counter is its position mod 32 (the level
// adds a multiple of 64).  The main kernels load 16 bytes per lane where the rows allow it (pitch a multiple of 16 bytes):
//   u8:  4 lanes per row, 16 rows per wave, 8 per 32-lane bank group.  Lane (s, l) of a group, s its row, holds words
//        k = 0..3 of columns 16 l + 4 k + j.  At unrolled step (k, j) it counts word (k + s) mod 4, byte (j + (s >> 2)) mod 4
//        (its registers are rotated once per load): bank 16 ((j + (s >> 2)) & 1) + 4 ((k + s) & 3) + l -- the 32 lanes of
//        a group on 32 banks.
//   f32: 16 lanes per row (lane 4 l + k holds columns 16 l + 4 k + j), 4 rows per wave, 2 per group; the odd row of a group
//        rotates its four elements by one: bank 16 ((j + s) & 1) + 4 k + l, again 32 lanes on 32 banks.
// The _narrow kernels read element by element (any pitch and base): a wave covers 64 / lw rows of lw = the tile's width
// rounded up to a power of two lanes; at lw = 64 lane m takes column rev(m), position m.  A partial 16-byte group of the
// last tile is read element by element too, so no load passes the row's width.
//
// fsea_persist_image and fsea_persist_decay_u32 stream over the counts: 16 pixels (four 16-byte loads, one 16-byte store) per
// lane where the width is a multiple of 16, one pixel otherwise; four counts per lane (256 width is a multiple of 4).
#include "fsea_rows.h"

#include <cmath>

using fsea_detail::DeviceGuard;
using fsea_detail::fail;
using fsea_detail::run_of_workgroup;

namespace {

constexpr int PS_WG = 256;                       // lanes per workgroup
constexpr int PS_C = 64;                         // columns per tile
constexpr int PS_L = FSEA_PERSIST_LEVELS;        // levels
constexpr int PS_RUN = FSEA_PERSIST_RUN_ROWS;    // rows per workgroup
static_assert(PS_L * PS_C * sizeof(uint32_t) <= 80 * 1024, "two workgroups per CU");
static_assert(PS_RUN % 64 == 0, "a run is whole iterations of the u8 kernel (64 rows) and the f32 kernel (16 rows)");

struct Range {
    float lo, scale;
};

// the position of column c of a tile in a level's row of the histogram, and back: the base-4 digits reversed
__device__ __forceinline__ uint32_t rev6(uint32_t c) { return (c & 3u) << 4 | (c & 12u) | c >> 4; }

// level of an f32 element: two rounded operations, no fused multiply-add; -1 for a NaN
__device__ __forceinline__ int level_f32(float v, Range r) {
    const float t = __fmul_rn(__fsub_rn(v, r.lo), r.scale);
    if (t != t) return -1;
    return t < 0.0f ? 0 : t >= 256.0f ? 255 : (int)t;
}

template <bool F32>
__device__ __forceinline__ int level_at(const void *__restrict__ rows, size_t i, Range r) {
    if (F32) return level_f32(static_cast<const float *>(rows)[i], r);
    return (int)static_cast<const uint8_t *>(rows)[i];
}

__device__ __forceinline__ void hist_zero(uint32_t *hist) {
    for (int i = threadIdx.x; i < PS_L * PS_C / 4; i += PS_WG) reinterpret_cast<uint4 *>(hist)[i] = uint4{0u, 0u, 0u, 0u};
    __syncthreads();
}

// the non-zero counters of the tile to counts[level * width + c0 + column]
__device__ __forceinline__ void hist_flush(const uint32_t *hist, uint32_t *__restrict__ counts, int width, int c0) {
    __syncthreads();
    for (int i = threadIdx.x; i < PS_L * PS_C / 4; i += PS_WG) {
        const uint4 h = reinterpret_cast<const uint4 *>(hist)[i];
        const int level = i >> 4;
        const uint32_t p0 = (uint32_t)(i & 15) << 2;      // positions p0 .. p0 + 3: columns rev6(p0) + 16 j
        uint32_t *dst = counts + (size_t)level * width + c0 + rev6(p0);
        if (h.x) atomicAdd(dst, h.x);
        if (h.y) atomicAdd(dst + 16, h.y);
        if (h.z) atomicAdd(dst + 32, h.z);
        if (h.w) atomicAdd(dst + 48, h.w);
    }
}

// One 16-byte group of a row: its four words rotated by the lane's row so that an unrolled step puts the 32 lanes of a
// bank group on 32 banks (the file's head).  `valid`: the row exists and the group lies inside the width.
struct Group {
    uint4 w;
    bool valid;
};

// u8: lane (row r of the wave's 16, l) counts columns 16 l .. 16 l + 15 of its row
__device__ __forceinline__ void count_u8(uint32_t *hist, Group g, uint32_t s, uint32_t l) {
    if (!g.valid) return;
    uint32_t w[4] = {g.w.x, g.w.y, g.w.z, g.w.w};
    const uint32_t wr = s & 3u, br = (s >> 2) & 1u;
    if (wr & 1u) { const uint32_t t = w[0]; w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = t; }
    if (wr & 2u) { uint32_t t = w[0]; w[0] = w[2]; w[2] = t; t = w[1]; w[1] = w[3]; w[3] = t; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t word = __builtin_rotateright32(w[k], 8u * br);   // byte j of it: byte (j + br) mod 4 of the row's word
        const uint32_t kk = (k + wr) & 3u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t jj = (j + br) & 3u;
            atomicAdd(&hist[((word >> (8 * j)) & 0xffu) * PS_C + (jj << 4 | kk << 2 | l)], 1u);
        }
    }
}

// f32: lane (row of the wave's 4, m = 4 l + k) counts columns 4 m .. 4 m + 3 of its row; nothing for a NaN
__device__ __forceinline__ void count_f32(uint32_t *hist, Group g, uint32_t s, uint32_t m, Range r) {
    if (!g.valid) return;
    uint32_t w[4] = {g.w.x, g.w.y, g.w.z, g.w.w};
    const uint32_t br = s & 1u;
    if (br) { const uint32_t t = w[0]; w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = t; }
    const uint32_t base = (m & 3u) << 2 | m >> 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int level = level_f32(__uint_as_float(w[j]), r);
        if (level >= 0) atomicAdd(&hist[level * PS_C + (((j + br) & 3u) << 4 | base)], 1u);
    }
}

// The 16-byte kernels.  pitch, in elements, is a multiple of EPG = 16 / the element size and `rows` is 16-byte aligned, so
// every group of a tile (c0 a multiple of 64) is aligned.
template <bool F32>
__device__ __forceinline__ void persist_body(const void *__restrict__ rows, size_t n_rows, size_t pitch, int width, Range r,
                                             uint32_t *__restrict__ counts) {
    constexpr int EPG = F32 ? 4 : 16;             // elements per group
    constexpr int LPR = PS_C / EPG;               // lanes per row
    constexpr int RPI = PS_WG / LPR;              // rows per iteration of the workgroup
    __shared__ __attribute__((aligned(16))) uint32_t hist[PS_L * PS_C];
    hist_zero(hist);

    const int tid = threadIdx.x;
    const int c0 = (int)blockIdx.y * PS_C;
    const uint32_t m = (uint32_t)tid % LPR;                    // the lane's group of the row
    const uint32_t s = ((uint32_t)tid / LPR) & (32 / LPR - 1);  // its row within the 32-lane bank group
    const int col = c0 + (int)m * EPG;
    size_t row0;
    const int run = run_of_workgroup<PS_RUN>(n_rows, &row0);
    const bool whole = col + EPG <= width;                     // a group that ends past the width is read by element
    const char *src = static_cast<const char *>(rows);
    const size_t esz = F32 ? 4 : 1;

    auto load = [&](int rr) {
        Group g;
        g.valid = whole && rr < run;
        g.w = uint4{0u, 0u, 0u, 0u};
        if (g.valid) g.w = *reinterpret_cast<const uint4 *>(src + ((row0 + rr) * pitch + col) * esz);
        return g;
    };
    auto count = [&](Group g) {
        if (F32) count_f32(hist, g, s, m, r);
        else count_u8(hist, g, s, m);
    };
    // two loads in flight
    for (int rr = tid / LPR; rr < run; rr += 2 * RPI) {
        const Group a = load(rr), b = load(rr + RPI);
        count(a);
        count(b);
    }
    if (!whole && col < width) {
        for (int rr = tid / LPR; rr < run; rr += RPI) {
            for (int e = 0; e < width - col; ++e) {
                const int level = level_at<F32>(rows, (row0 + rr) * pitch + col + e, r);
                if (level >= 0) atomicAdd(&hist[level * PS_C + rev6((uint32_t)(col - c0 + e))], 1u);
            }
        }
    }
    hist_flush(hist, counts, width, c0);
}

// Element by element: any pitch, any base.  lw_log2: the lanes of a row, the tile's width rounded up to a power of two.
template <bool F32>
__device__ __forceinline__ void persist_narrow_body(const void *__restrict__ rows, size_t n_rows, size_t pitch, int width,
                                                    int lw_log2, Range r, uint32_t *__restrict__ counts) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[PS_L * PS_C];
    hist_zero(hist);

    const int tid = threadIdx.x;
    const int c0 = (int)blockIdx.y * PS_C;
    const uint32_t cm = (uint32_t)tid & ((1u << lw_log2) - 1u);
    const uint32_t c = lw_log2 == 6 ? rev6(cm) : cm;           // 64 lanes per row: lane m at position m
    const int rpi = PS_WG >> lw_log2;
    size_t row0;
    const int run = run_of_workgroup<PS_RUN>(n_rows, &row0);
    if (c0 + (int)c < width) {
        const uint32_t pos = rev6(c);
        for (int rr = tid >> lw_log2; rr < run; rr += rpi) {
            const int level = level_at<F32>(rows, (row0 + rr) * pitch + c0 + c, r);
            if (level >= 0) atomicAdd(&hist[level * PS_C + pos], 1u);
        }
    }
    hist_flush(hist, counts, width, c0);
}

// the three maps of a count (include/fsea.h); q of the LOG map
__device__ __forceinline__ uint32_t log_q(uint32_t c) {
    const uint32_t e = 31u - (uint32_t)__clz((int)c);
    return 256u * e + (uint32_t)((((uint64_t)c << 8) >> e) & 255u) + 1u;
}

__device__ __forceinline__ uint32_t map_count(uint32_t c, int map, uint64_t full, uint32_t log_den) {
    if (map == FSEA_PERSIST_MAP_SATURATE) return min(c, 255u);
    if (c == 0u || full == 0u) return 0u;
    if (map == FSEA_PERSIST_MAP_LINEAR) {
        const uint64_t v = (uint64_t)c * 255u / full;
        return v > 255u ? 255u : (uint32_t)v;
    }
    return min(255u, 1u + (log_q(c) - 1u) * 254u / log_den);
}

__device__ __forceinline__ uint32_t map4(uint4 c, int map, uint64_t full, uint32_t log_den) {
    return map_count(c.x, map, full, log_den) | map_count(c.y, map, full, log_den) << 8 |
           map_count(c.z, map, full, log_den) << 16 | map_count(c.w, map, full, log_den) << 24;
}

}  // namespace

extern "C" __global__ __launch_bounds__(PS_WG) void fsea_persist_u8(const void *__restrict__ rows, size_t n_rows, size_t pitch,
                                                                    int width, uint32_t *__restrict__ counts) {
    persist_body<false>(rows, n_rows, pitch, width, Range{0.0f, 0.0f}, counts);
}
extern "C" __global__ __launch_bounds__(PS_WG) void fsea_persist_f32(const void *__restrict__ rows, size_t n_rows, size_t pitch,
                                                                     int width, float lo, float scale,
                                                                     uint32_t *__restrict__ counts) {
    persist_body<true>(rows, n_rows, pitch, width, Range{lo, scale}, counts);
}
extern "C" __global__ __launch_bounds__(PS_WG) void fsea_persist_u8_narrow(const void *__restrict__ rows, size_t n_rows,
                                                                           size_t pitch, int width, int lw_log2,
                                                                           uint32_t *__restrict__ counts) {
    persist_narrow_body<false>(rows, n_rows, pitch, width, lw_log2, Range{0.0f, 0.0f}, counts);
}
extern "C" __global__ __launch_bounds__(PS_WG) void fsea_persist_f32_narrow(const void *__restrict__ rows, size_t n_rows,
                                                                            size_t pitch, int width, int lw_log2, float lo,
                                                                            float scale, uint32_t *__restrict__ counts) {
    persist_narrow_body<true>(rows, n_rows, pitch, width, lw_log2, Range{lo, scale}, counts);
}

// image[(255 - l) * width + k] = map(counts[l * width + k]).  vec != 0 (width a multiple of 16): 16 pixels per lane,
// n = 16 width groups; otherwise one pixel per lane, n = 256 width pixels.
extern "C" __global__ __launch_bounds__(PS_WG) void fsea_persist_image(const uint32_t *__restrict__ counts, int width, int vec,
                                                                       long long n, int map, uint64_t full, uint32_t log_den,
                                                                       uint8_t *__restrict__ image) {
    const long long i = (long long)blockIdx.x * PS_WG + threadIdx.x;
    if (i >= n) return;
    if (vec) {
        const int gpr = width >> 4;                           // groups per row
        const int level = (int)(i / gpr), g = (int)(i - (long long)level * gpr);
        const uint4 *src = reinterpret_cast<const uint4 *>(counts + (size_t)level * width) + 4 * g;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = map4(src[j], map, full, log_den);
        reinterpret_cast<uint4 *>(image + (size_t)(PS_L - 1 - level) * width)[g] = uint4{w[0], w[1], w[2], w[3]};
    } else {
        const int level = (int)(i / width), k = (int)(i - (long long)level * width);
        image[(size_t)(PS_L - 1 - level) * width + k] = (uint8_t)map_count(counts[i], map, full, log_den);
    }
}

// c <- floor(c * numerator / denominator), four counts per lane: n = 64 width groups
extern "C" __global__ __launch_bounds__(PS_WG) void fsea_persist_decay_u32(uint4 *__restrict__ counts, long long n,
                                                                           uint32_t numerator, uint32_t denominator) {
    const long long i = (long long)blockIdx.x * PS_WG + threadIdx.x;
    if (i >= n) return;
    uint4 c = counts[i];
    c.x = (uint32_t)((uint64_t)c.x * numerator / denominator);
    c.y = (uint32_t)((uint64_t)c.y * numerator / denominator);
    c.z = (uint32_t)((uint64_t)c.z * numerator / denominator);
    c.w = (uint32_t)((uint64_t)c.w * numerator / denominator);
    counts[i] = c;
}

// `rows` is scaled by every decay
struct fsea_persist : fsea_detail::RowObject {
    float lo = -100.0f, hi = 0.0f, scale = 2.56f;
    fsea_detail::ZeroedScratch counts;            // 256 x width u32, level-major; its event orders the calls
    std::mutex mu;
    fsea_detail::HostStaging staging;             // the host forms
};

namespace {

uint64_t host_log_q(uint64_t c) {
    if (!c) return 0;
    int e = 63;
    while (!(c >> e)) --e;
    const uint64_t m = (e >= 8 ? c >> (e - 8) : c << (8 - e)) & 255u;
    return 256u * (uint64_t)e + m + 1u;
}

int check_image(const fsea_persist *p, int map, const void *image) {
    if (!p) return fail(FSEA_EINVAL, "persist is NULL");
    if (map != FSEA_PERSIST_MAP_SATURATE && map != FSEA_PERSIST_MAP_LINEAR && map != FSEA_PERSIST_MAP_LOG) {
        return fail(FSEA_EINVAL, "unknown map %d", map);
    }
    if (!image) return fail(FSEA_EINVAL, "image is NULL");
    return FSEA_OK;
}

// One add on device rows, asynchronous on `s`.  The caller holds p->mu, is on p's device and has checked the arguments.
int add_launch(fsea_persist *p, const void *d_rows, int type, size_t n_rows, size_t pitch, hipStream_t s) {
    int rc = p->counts.acquire(s);
    if (rc) return rc;
    uint32_t *counts = static_cast<uint32_t *>(p->counts.buf.ptr);
    const int width = p->width;
    const dim3 grid((unsigned)((n_rows + PS_RUN - 1) / PS_RUN), (unsigned)((width + PS_C - 1) / PS_C));
    const size_t esz = fsea_detail::row_elem_bytes(type);
    const bool vec = fsea_detail::rows_vec16(d_rows, pitch * esz) && (size_t)width * esz >= 16;
    int lw_log2 = 0;
    while ((1 << lw_log2) < std::min(width, PS_C)) ++lw_log2;
    if (type == FSEA_PERSIST_U8) {
        if (vec) hipLaunchKernelGGL(fsea_persist_u8, grid, dim3(PS_WG), 0, s, d_rows, n_rows, pitch, width, counts);
        else hipLaunchKernelGGL(fsea_persist_u8_narrow, grid, dim3(PS_WG), 0, s, d_rows, n_rows, pitch, width, lw_log2, counts);
    } else {
        if (vec) hipLaunchKernelGGL(fsea_persist_f32, grid, dim3(PS_WG), 0, s, d_rows, n_rows, pitch, width, p->lo, p->scale, counts);
        else hipLaunchKernelGGL(fsea_persist_f32_narrow, grid, dim3(PS_WG), 0, s, d_rows, n_rows, pitch, width, lw_log2, p->lo, p->scale, counts);
    }
    FSEA_HIP(hipGetLastError());
    p->rows += n_rows;
    return p->counts.release(s);
}

int image_launch(fsea_persist *p, int map, uint64_t full, uint8_t *d_image, hipStream_t s) {
    if (full == 0) full = p->rows;
    const uint64_t qf = host_log_q(full);
    const uint32_t log_den = (uint32_t)std::max<uint64_t>(1, qf ? qf - 1 : 0);
    int rc = p->counts.acquire(s);
    if (rc) return rc;
    const int vec = p->width % 16 == 0;
    const long long n = vec ? (long long)PS_L * (p->width / 16) : (long long)PS_L * p->width;
    hipLaunchKernelGGL(fsea_persist_image, dim3((unsigned)((n + PS_WG - 1) / PS_WG)), dim3(PS_WG), 0, s,
                       static_cast<const uint32_t *>(p->counts.buf.ptr), p->width, vec, n, map, full, log_den, d_image);
    FSEA_HIP(hipGetLastError());
    return p->counts.release(s);
}

}  // namespace

extern "C" {

int fsea_persist_create(fsea_persist **out, int width, int device) {
    if (!out) return fail(FSEA_EINVAL, "persist out-pointer is NULL");
    *out = nullptr;
    if (width < 1 || width > FSEA_PERSIST_MAX_WIDTH) {
        return fail(FSEA_EINVAL, "width must be in [1, %d], got %d", FSEA_PERSIST_MAX_WIDTH, width);
    }
    return fsea_detail::create_object(out, device, "fsea_persist_create", [&](fsea_persist *p) -> int {
        p->width = width;
        return p->counts.create_zeroed("fsea_persist_create", (size_t)PS_L * width * sizeof(uint32_t), p->staging.stream);
    });
}

int fsea_persist_destroy(fsea_persist *p) { return fsea_detail::destroy_object(p); }

int fsea_persist_reset(fsea_persist *p) {
    return fsea_detail::reset_object(p, "persist is NULL", [&] {
        p->rows = 0;
        return p->counts.zero();
    });
}

int fsea_persist_set_range(fsea_persist *p, float lo, float hi) {
    if (!p) return fail(FSEA_EINVAL, "persist is NULL");
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) {
        return fail(FSEA_EINVAL, "the range must be finite with lo < hi, got (%g, %g)", (double)lo, (double)hi);
    }
    const float scale = (float)(256.0 / ((double)hi - (double)lo));
    if (!std::isfinite(scale)) return fail(FSEA_EINVAL, "the range (%g, %g) is too narrow for an f32 scale", (double)lo, (double)hi);
    std::lock_guard<std::mutex> lock(p->mu);
    p->lo = lo;
    p->hi = hi;
    p->scale = scale;
    return FSEA_OK;
}

int fsea_persist_width(const fsea_persist *p) { return p ? p->width : 0; }

uint64_t fsea_persist_rows(const fsea_persist *p) { return p ? p->rows : 0; }

int fsea_persist_add_device(fsea_persist *p, const void *d_rows, int type, size_t n_rows, size_t pitch, void *stream) {
    int rc = fsea_detail::check_rows_add(p, "persist", d_rows, type, n_rows, pitch);
    if (!rc && n_rows) rc = fsea_detail::check_aligned16("d_rows", d_rows);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = fsea_detail::check_rows_room(p, n_rows))) return rc;
    FSEA_ON_DEVICE(p->device);
    return add_launch(p, d_rows, type, n_rows, pitch, static_cast<hipStream_t>(stream));
}

int fsea_persist_add_host(fsea_persist *p, const void *rows, int type, size_t n_rows, size_t pitch) {
    int rc = fsea_detail::check_rows_add(p, "persist", rows, type, n_rows, pitch);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(p->mu);
    if ((rc = fsea_detail::check_rows_room(p, n_rows))) return rc;
    FSEA_ON_DEVICE(p->device);
    // the rows go up packed, in chunks
    const size_t esz = fsea_detail::row_elem_bytes(type);
    const fsea_detail::PackedPlane in(rows, pitch * esz, (size_t)p->width * esz);
    return fsea_detail::for_row_chunks(n_rows, in.packed, [&](size_t r0, size_t nr) {
        return p->staging.run(
            nr * in.packed, 0, nullptr, [&](void *h_in) { in.pack(h_in, r0, nr); },
            [&](void *d_in, void *, hipStream_t s) { return add_launch(p, d_in, type, nr, in.packed / esz, s); });
    });
}

int fsea_persist_decay(fsea_persist *p, uint32_t numerator, uint32_t denominator, void *stream) {
    if (!p) return fail(FSEA_EINVAL, "persist is NULL");
    if (denominator < 1 || numerator > denominator) {
        return fail(FSEA_EINVAL, "the decay ratio needs 1 <= denominator and numerator <= denominator, got %u / %u", numerator,
                    denominator);
    }
    std::lock_guard<std::mutex> lock(p->mu);
    if (numerator == denominator) return FSEA_OK;
    FSEA_ON_DEVICE(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = p->counts.acquire(s);
    if (rc) return rc;
    const long long n = (long long)(PS_L / 4) * p->width;
    hipLaunchKernelGGL(fsea_persist_decay_u32, dim3((unsigned)((n + PS_WG - 1) / PS_WG)), dim3(PS_WG), 0, s,
                       static_cast<uint4 *>(p->counts.buf.ptr), n, numerator, denominator);
    FSEA_HIP(hipGetLastError());
    p->rows = p->rows * numerator / denominator;
    return p->counts.release(s);
}

int fsea_persist_counts_host(fsea_persist *p, uint32_t *counts) {
    if (!p) return fail(FSEA_EINVAL, "persist is NULL");
    if (!counts) return fail(FSEA_EINVAL, "counts is NULL");
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return p->counts.fetch(p->staging, counts);
}

int fsea_persist_image_device(fsea_persist *p, int map, uint64_t full, uint8_t *d_image, void *stream) {
    int rc = check_image(p, map, d_image);
    if (!rc) rc = fsea_detail::check_aligned16("d_image", d_image);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return image_launch(p, map, full, d_image, static_cast<hipStream_t>(stream));
}

int fsea_persist_image_host(fsea_persist *p, int map, uint64_t full, uint8_t *image) {
    int rc = check_image(p, map, image);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return p->staging.run(0, (size_t)PS_L * p->width, image, [](void *) {}, [&](void *, void *d_out, hipStream_t s) {
        return image_launch(p, map, full, static_cast<uint8_t *>(d_out), s);
    });
}

int fsea_persist_trace(const uint32_t *counts, int width, int kind, double fraction, uint8_t *levels) {
    if (!counts || !levels) return fail(FSEA_EINVAL, "NULL buffer");
    if (width < 1 || width > FSEA_PERSIST_MAX_WIDTH) {
        return fail(FSEA_EINVAL, "width must be in [1, %d], got %d", FSEA_PERSIST_MAX_WIDTH, width);
    }
    if (kind != FSEA_PERSIST_TRACE_MAX && kind != FSEA_PERSIST_TRACE_MIN && kind != FSEA_PERSIST_TRACE_QUANTILE) {
        return fail(FSEA_EINVAL, "unknown trace kind %d", kind);
    }
    if (kind == FSEA_PERSIST_TRACE_QUANTILE && !(fraction >= 0.0 && fraction <= 1.0)) {
        return fail(FSEA_EINVAL, "fraction must be in [0, 1], got %g", fraction);
    }
    for (int k = 0; k < width; ++k) {
        int level = 0;
        if (kind == FSEA_PERSIST_TRACE_MAX) {
            for (int l = PS_L - 1; l > 0 && !level; --l) level = counts[(size_t)l * width + k] ? l : 0;
        } else if (kind == FSEA_PERSIST_TRACE_MIN) {
            for (int l = 0; l < PS_L; ++l) {
                if (counts[(size_t)l * width + k]) {
                    level = l;
                    break;
                }
            }
        } else {
            uint64_t total = 0, sum = 0;
            for (int l = 0; l < PS_L; ++l) total += counts[(size_t)l * width + k];
            const uint64_t target = std::max<uint64_t>(1, (uint64_t)std::ceil(fraction * (double)total));
            for (int l = 0; l < PS_L && total; ++l) {
                sum += counts[(size_t)l * width + k];
                if (sum >= target) {
                    level = l;
                    break;
                }
            }
        }
        levels[k] = (uint8_t)level;
    }
    return FSEA_OK;
}

}  // extern "C"
