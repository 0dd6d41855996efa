// fsea_cfar.hip -- the CFAR spectrum detector (include/fsea.h: fsea_cfar_*): which cells of a dB row stand above the mean
// level of their neighbours, per-column hit counts over all the rows offered (the occupancy), and the bands of occupied
// columns.  Integer and order-free like the persistence spectrum (fsea_persist.hip): every mask byte, row count and hit
// count is the same whatever the launch geometry or the cut of the rows into calls.
//
// Kernels fsea_cfar_u8 / fsea_cfar_f32 (and their _narrow forms; DESIGN.md section 4, "The CFAR detector"): a workgroup of
// 256 lanes owns a tile of FSEA_CFAR_TILE_COLUMNS = 1024 columns and a run of FSEA_CFAR_RUN_ROWS = 64 rows; each of its four
// waves takes every fourth row of the run.  Per row a wave
//   1. stages the segment [a0, e1) of the row: the tile plus a halo of G + T cells each side, clipped at the row's ends, a0
//      rounded down to a multiple of 16 cells.  A lane loads 16 bytes (16 u8 or 4 f32 cells), turns them into levels, scans
//      them, the wave scans the lanes' totals (six __shfl_up steps) and a carry joins the chunks of 64 lanes.  The inclusive
//      prefix sums go to LDS as u32, q[FRONT + c - a0] for cell c, behind FRONT zero dwords (the cells before the row and the
//      cell before the segment); cells past the row's end have level 0, so the prefix stays constant there.  The tile's own
//      levels go to x[c - c0].
//   2. decides its 1024 cells in 16 steps of 64 consecutive columns: lane l takes column c0 + 64 j + l at step j.  A side sum
//      is the difference of two prefix values, so the cost per cell does not depend on T: four prefix reads at the fixed
//      offsets -G-T-1, -G-1, +G, +G+T from k (never clamped: the zeroes in front and the constant tail clip a window at the
//      row's ends) and one level read, every one 64 consecutive dwords across the wave -- 32 lanes of a bank group on 32
//      banks whatever G and T are.
//   3. the 64 decisions of a step are one ballot: its population count is the step's share of the row's hits, the lane keeps
//      its own bit in a register counter of column 64 j + l (the same 16 columns over all rows of the run), and lane m keeps
//      the 16 bits of columns 16 m .. 16 m + 15, which it spreads into 16 mask bytes and stores at once.
// At the end of the run the four waves add their column counters in LDS and the workgroup issues one u32 global atomic per
// non-zero column; a row's hits are one atomic per row and tile on row_hits, which the launch zeroes first.  The prefix and
// level arrays are a wave's own, so the four waves meet only at the kernel's first and last barrier, and a wave loads the
// 16-byte groups of its next row before it decides the current one.
//
// fsea_cfar_shared.h has what this file shares with fsea_oscfar.hip as code: the geometry's constants, level_at, spread4,
// wave_sync, the kernels' one signature, the object, its launch and the entry points.  Step 3 and the end of the run stand
// in both files as text: moved into functions they compile to other registers here ("What the detectors share").
//
// The prefix sums are u32 and wrap: an f32 level is in [-2^20, 2^20], so a prefix value may be "negative" (two's complement)
// or, over a long row, pass 2^32.  A side sum has at most 256 terms, |S| <= 2^28, and the difference of two u32 prefix values
// is that sum modulo 2^32, hence exact once read as an int32_t.  (Here the prefix restarts at every segment of at most 1680
// cells, so it stays below 2^31 in size; nothing depends on that.)
//
// The _narrow kernels are the same code with every cell loaded on its own (any pitch and base).  In the 16-byte kernels a
// group that would end past the row's width is loaded cell by cell too, so no load passes the width; the mask is written 16
// bytes per lane where the width is a multiple of 16 and byte by byte otherwise.
#include "fsea_cfar_shared.h"

#include <cmath>
#include <type_traits>

using fsea_detail::cfar_level_f32;
using fsea_detail::fail;
using fsea_detail::level_at;
using fsea_detail::run_of_workgroup;
using fsea_detail::spread4;
using fsea_detail::wave_sync;

namespace {

constexpr int CF_WAVES = fsea_detail::DET_WAVES;
constexpr int CF_C = fsea_detail::DET_C;          // columns per tile
constexpr int CF_HALO = FSEA_CFAR_MAX_GUARD + FSEA_CFAR_MAX_TRAIN;
constexpr int CF_SEG = CF_C + 2 * CF_HALO + 16;   // cells of a staged segment at most (a0 is rounded down by up to 15)
constexpr int CF_FRONT = (CF_HALO + 1 + 15) & ~15;   // zero dwords in front of a wave's prefix array: the cells before the row
constexpr int CF_Q = CF_FRONT + CF_SEG;           // dwords of a wave's prefix array
static_assert(CF_SEG % 16 == 0, "whole 16-byte groups");
static_assert((CF_WAVES * (CF_Q + CF_C) + CF_C) * 4 <= 80 * 1024, "two workgroups per CU");

struct Settings {
    int guard = 2, train = 16, offset = 60, method = FSEA_CFAR_CA;
};

// Whether the group that starts at `cell` is read with one 16-byte load: the kernel may (VEC), the group starts inside the
// segment and ends inside the width.
template <bool VEC, int EPG>
__device__ __forceinline__ bool whole_group(int cell, int end, int width) {
    return VEC && cell < end && cell + EPG <= width;
}

// The EPG levels of the group that starts at cell `cell` of the row at element offset `at`: from `w`, its 16 bytes loaded
// ahead, where whole_group() holds; cell by cell below `end` otherwise; 0 for what is not loaded.
template <bool F32, bool VEC, int EPG>
__device__ __forceinline__ void levels_of(const void *__restrict__ rows, size_t at, int cell, int end, int width, bool live,
                                          uint4 w, int (&lv)[EPG]) {
    if (whole_group<VEC, EPG>(cell, end, width)) {
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < EPG; ++e) {
            if (F32) lv[e] = live ? cfar_level_f32(__uint_as_float(ws[e & 3])) : 0;
            else lv[e] = (int)((ws[e >> 2] >> (8 * (e & 3))) & 0xffu);
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < EPG; ++e) lv[e] = live && cell + e < end ? level_at<F32>(rows, at + cell + e) : 0;
}

template <bool F32, bool VEC>
__device__ __forceinline__ void cfar_body(const void *__restrict__ rows, size_t n_rows, size_t pitch, int width, Settings st,
                                          uint8_t *__restrict__ mask, int mask_vec, uint32_t *__restrict__ row_hits,
                                          uint32_t *__restrict__ hits) {
    constexpr int EPG = F32 ? 4 : 16;             // elements per 16-byte group
    __shared__ __attribute__((aligned(16))) uint32_t q_all[CF_WAVES][CF_Q];
    __shared__ __attribute__((aligned(16))) int32_t x_all[CF_WAVES][CF_C];
    __shared__ uint32_t total[CF_C];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *q = q_all[wave];
    int32_t *x = x_all[wave];
    const int c0 = (int)blockIdx.y * CF_C;
    const int G = st.guard, T = st.train;
    const int a0 = max(0, c0 - G - T) & ~15;                   // the segment [a0, e1) of the row ...
    const int e1 = min(width, c0 + CF_C + G + T);
    const int ngrp = (c0 + CF_C + G + T - a0 + EPG - 1) / EPG; // ... and the groups up to the last cell a window may name
    const bool inner = c0 - G - T >= 0 && c0 + CF_C + G + T <= width;
    size_t row0;
    const int run = run_of_workgroup<fsea_detail::DET_RUN>(n_rows, &row0);

    for (int i = tid; i < CF_C; i += fsea_detail::DET_WG) total[i] = 0u;
    for (int i = lane; i < CF_FRONT; i += 64) q[i] = 0u;       // the cells before the row and before the segment
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};                        // the lane's 16 columns, a byte each: at most DET_RUN / 4 hits
    __syncthreads();

    // the 16-byte groups of a row are loaded one row ahead: raw[c] is the lane's group of chunk c (zero where there is none)
    constexpr int NCH = (CF_SEG / EPG + 63) / 64;
    uint4 raw[NCH];
    auto fetch = [&](int rr, int zero) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int cell = a0 + (c * 64 + lane + zero) * EPG;
            raw[c] = uint4{0u, 0u, 0u, 0u};
            if (rr < run && whole_group<VEC, EPG>(cell, e1, width)) {
                raw[c] = *reinterpret_cast<const uint4 *>(static_cast<const char *>(rows) +
                                                          ((row0 + rr) * pitch + cell) * (F32 ? 4 : 1));
            }
        }
    };
    fetch(wave, 0);

    for (int it = 0; it < (run + CF_WAVES - 1) / CF_WAVES; ++it) {
        const int rr = it * CF_WAVES + wave;
        const bool live = rr < run;
        const size_t row = row0 + (live ? rr : 0);
        // 0, behind an asm the compiler cannot see through: what depends on the lane and the column alone (which groups are
        // whole, which lie in the tile, the windows' counts at the row's ends, the step that holds the lane's mask bits)
        // is worked out again in every row.  Hoisted out of the row loop for all chunks and all 16 steps at once it costs
        // more registers than the kernel has.
        int zero;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zero));

        // 1. the segment's levels and their inclusive prefix sums
        uint32_t carry = 0u;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (c * 64 >= ngrp) break;
            const int g = c * 64 + lane + zero;
            const int cell = a0 + g * EPG;
            int lv[EPG];
            levels_of<F32, VEC, EPG>(rows, row * pitch, cell, e1, width, live, raw[c], lv);
            uint32_t p[EPG], s = 0u;
#pragma unroll
            for (int e = 0; e < EPG; ++e) {
                s += (uint32_t)lv[e];
                p[e] = s;
            }
            uint32_t t = s;                                    // the wave's inclusive scan of the lanes' totals
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(t, d);
                t += up & (uint32_t)((d - 1 - lane) >> 31);    // lanes d and up; a mask in a register, not a saved exec
            }
            const uint32_t base = carry + t - s;
            carry += __shfl(t, 63);
            if (g < ngrp) {
                uint4 *dst = reinterpret_cast<uint4 *>(q + CF_FRONT + g * EPG);
#pragma unroll
                for (int e = 0; e < EPG; e += 4) dst[e >> 2] = uint4{p[e] + base, p[e + 1] + base, p[e + 2] + base, p[e + 3] + base};
                if (cell >= c0 && cell < c0 + CF_C) {          // a0 and c0 are multiples of 16: a group is inside or outside
                    int4 *xd = reinterpret_cast<int4 *>(x + (cell - c0));
#pragma unroll
                    for (int e = 0; e < EPG; e += 4) xd[e >> 2] = int4{lv[e], lv[e + 1], lv[e + 2], lv[e + 3]};
                }
            }
        }
        fetch(rr + CF_WAVES, zero);                            // the next row's loads fly while this one is decided
        wave_sync();

        // 2. the decisions: column c0 + 64 j + lane at step j
        // No index is clamped: the zeroes in front of the segment and the constant prefix behind the row's end make a
        // clipped window's difference the clipped sum, so the four streams are qk + a fixed offset + 64 j.
        const uint32_t *qk = q + CF_FRONT + (c0 - a0) + lane;  // qk[i]: the prefix value of cell c0 + lane + i
        uint32_t mybits = 0u, rh = 0u;
        // A tile whose windows all lie inside the row (`inner`) has nL = nR = T everywhere; in the other tiles the counts
        // depend on the column (with `zero`: see the head of the loop).
        const int is_ca = -(int)(st.method == FSEA_CFAR_CA), is_go = -(int)(st.method == FSEA_CFAR_GO), is_so = ~(is_ca | is_go);
        auto decide = [&](auto edge) {
            constexpr bool EDGE = decltype(edge)::value;
            const int own = (lane >> 2) + zero;                // the step whose ballot holds the lane's 16 mask bits
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int kk = 64 * j + lane, k = c0 + kk + (EDGE ? zero : 0);
                const int xl = x[kk];
                const int nL = EDGE ? min(max(k - G, 0), T) : T, nR = EDGE ? min(max(width - 1 - k - G, 0), T) : T;
                const int SL = (int)(qk[64 * j - G - 1] - qk[64 * j - G - T - 1]);   // exact: the u32 difference is the sum
                const int SR = (int)(qk[64 * j + G + T] - qk[64 * j + G]);           // modulo 2^32, and |sum| <= 2^28
                const int dL = xl * nL - SL - st.offset * nL, dR = xl * nR - SR - st.offset * nR;   // 0 for an empty side
                // GO: an empty side (d = 0) stands back for the other; both empty: 0, no hit
                const int gL = EDGE && nL == 0 ? dR : dL, gR = EDGE && nR == 0 ? dL : dR;
                const int v = ((dL + dR) & is_ca) | (min(gL, gR) & is_go) | (max(dL, dR) & is_so);   // one code path for the three
                bool hit = v > 0;
                hit = hit && live && (!EDGE || k < width);
                if (mask && !mask_vec && live && (!EDGE || k < width)) mask[row * (size_t)width + k] = hit ? 255 : 0;
                const unsigned long long b = __ballot(hit);
                rh += (uint32_t)__popcll(b);
                cnt[j >> 2] += (hit ? 1u : 0u) << (8 * (j & 3));
                if (own == j) mybits = (uint32_t)(b >> (16 * (lane & 3))) & 0xffffu;
            }
        };
        if (inner) decide(std::false_type{});
        else decide(std::true_type{});
        if (live) {
            const int col = c0 + 16 * lane;
            if (mask && mask_vec && col < width) {             // width is a multiple of 16: the group is inside
                *reinterpret_cast<uint4 *>(mask + row * (size_t)width + col) =
                    uint4{spread4(mybits), spread4(mybits >> 4), spread4(mybits >> 8), spread4(mybits >> 12)};
            }
            if (row_hits && lane == 0 && rh) atomicAdd(&row_hits[row], rh);
        }
        wave_sync();                                           // before the next row overwrites q and x
    }

    // 3. the run's column hits: the four waves in LDS, then one global atomic per non-zero column
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t n = (cnt[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (n) atomicAdd(&total[64 * j + lane], n);
    }
    __syncthreads();
    for (int i = tid; i < CF_C; i += fsea_detail::DET_WG) {
        const uint32_t v = total[i];
        if (v && c0 + i < width) atomicAdd(&hits[c0 + i], v);
    }
}

}  // namespace

FSEA_DETECTOR_KERNEL(fsea_cfar_u8, cfar_body, 3, false, true)
FSEA_DETECTOR_KERNEL(fsea_cfar_f32, cfar_body, 3, true, true)
FSEA_DETECTOR_KERNEL(fsea_cfar_u8_narrow, cfar_body, 3, false, false)
FSEA_DETECTOR_KERNEL(fsea_cfar_f32_narrow, cfar_body, 3, true, false)

// object, launch and entry points: fsea_cfar_shared.h
struct fsea_cfar : fsea_detail::Detector<Settings, fsea_cfar_u8, fsea_cfar_f32, fsea_cfar_u8_narrow, fsea_cfar_f32_narrow> {};

extern "C" {

int fsea_cfar_create(fsea_cfar **out, int width, int device) {
    return fsea_detail::detector_create(out, width, device, "cfar", "fsea_cfar_create");
}

int fsea_cfar_destroy(fsea_cfar *c) { return fsea_detail::destroy_object(c); }

int fsea_cfar_reset(fsea_cfar *c) { return fsea_detail::detector_reset(c, "cfar is NULL"); }

int fsea_cfar_set(fsea_cfar *c, int guard, int train, int offset, int method) {
    if (int rc = fsea_detail::detector_check_set(c, "cfar", guard, train, offset)) return rc;
    if (method != FSEA_CFAR_CA && method != FSEA_CFAR_GO && method != FSEA_CFAR_SO) return fail(FSEA_EINVAL, "unknown method %d", method);
    std::lock_guard<std::mutex> lock(c->mu);
    c->set = Settings{guard, train, offset, method};
    return FSEA_OK;
}

int fsea_cfar_width(const fsea_cfar *c) { return c ? c->width : 0; }

uint64_t fsea_cfar_rows(const fsea_cfar *c) { return c ? c->rows : 0; }

int fsea_cfar_add_device(fsea_cfar *c, const void *d_rows, int type, size_t n_rows, size_t pitch, uint8_t *d_mask,
                         uint32_t *d_row_hits, void *stream) {
    return fsea_detail::detector_add_device(c, "cfar", d_rows, type, n_rows, pitch, d_mask, d_row_hits, stream);
}

int fsea_cfar_add_host(fsea_cfar *c, const void *rows, int type, size_t n_rows, size_t pitch, uint8_t *mask, uint32_t *row_hits) {
    return fsea_detail::detector_add_host(c, "cfar", rows, type, n_rows, pitch, mask, row_hits);
}

int fsea_cfar_hits_host(fsea_cfar *c, uint32_t *hits) { return fsea_detail::detector_hits_host(c, "cfar", hits); }

int fsea_cfar_bands(const uint32_t *hits, int width, uint64_t rows, double min_fraction, int max_gap, int min_width,
                    fsea_cfar_band *bands, size_t capacity, size_t *n_bands) {
    if (!hits || !n_bands || (!bands && capacity)) return fail(FSEA_EINVAL, "NULL buffer");
    if (width < 1 || width > FSEA_CFAR_MAX_WIDTH) {
        return fail(FSEA_EINVAL, "width must be in [1, %d], got %d", FSEA_CFAR_MAX_WIDTH, width);
    }
    if (!(min_fraction >= 0.0 && min_fraction <= 1.0)) return fail(FSEA_EINVAL, "min_fraction must be in [0, 1], got %g", min_fraction);
    if (max_gap < 0) return fail(FSEA_EINVAL, "max_gap must not be negative, got %d", max_gap);
    if (min_width < 1) return fail(FSEA_EINVAL, "min_width must be at least 1, got %d", min_width);
    size_t found = 0;
    *n_bands = 0;
    if (rows == 0) return FSEA_OK;
    const uint64_t c_min = std::max<uint64_t>(1, (uint64_t)std::ceil(min_fraction * (double)rows));
    auto close_band = [&](int first, int last) {
        if (last - first + 1 < min_width) return;
        if (found < capacity) {
            fsea_cfar_band b{first, last, first, hits[first], 0};
            for (int k = first; k <= last; ++k) {
                b.hits_sum += hits[k];
                if (hits[k] > b.peak_hits) {
                    b.peak = k;
                    b.peak_hits = hits[k];
                }
            }
            bands[found] = b;
        }
        ++found;
    };
    int first = -1, last = -1;
    for (int k = 0; k < width; ++k) {
        if (hits[k] < c_min) continue;
        if (first >= 0 && k - last - 1 > max_gap) {
            close_band(first, last);
            first = -1;
        }
        if (first < 0) first = k;
        last = k;
    }
    if (first >= 0) close_band(first, last);
    *n_bands = found;
    return FSEA_OK;
}

}  // extern "C"
