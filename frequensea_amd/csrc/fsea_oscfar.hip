// fsea_oscfar.hip -- the ordered-statistic CFAR detector (include/fsea.h: fsea_oscfar_*): which cells of a dB row stand
// above the R-th smallest level of their training cells, per-column hit counts over all the rows offered, and the row hits.
// Where fsea_cfar (fsea_cfar.hip) compares a cell with the mean of its neighbours, which a strong neighbour pulls up, this
// one compares it with a rank of them: the weaker of two close carriers keeps its hit.  Integer and order-free like the
// objects around it: every mask byte, row count and hit count is the same whatever the launch geometry or the cut of the
// rows into calls.  Levels, windows, counts and the accounting of mask, hits, row hits and rows are fsea_cfar's.
//
// The decision needs no sort.  With r = ceil(R n / 2T), "x > z + offset for the r-th smallest level z of the n training
// cells" says the same as "at least r training cells have level + offset < x": if r cells lie below x - offset, the r-th
// smallest does; if the r-th smallest does, so do the r - 1 before it.  And count >= ceil(R n / 2T) is count * 2T >= R n
// in integers, so the kernel divides nothing.
//
// Kernels fsea_oscfar_u8 / fsea_oscfar_f32 (and their _narrow forms; DESIGN.md section 4, "The ordered-statistic CFAR"): the
// geometry and the epilogue are fsea_cfar's.  A workgroup of 256 lanes owns a tile of FSEA_OSCFAR_TILE_COLUMNS = 1024 columns
// and a run of FSEA_OSCFAR_RUN_ROWS = 64 rows; each of its four waves takes every fourth row of the run.  Per row a wave
//   1. stages the levels of the tile and of a halo of G + T cells each side (rounded up to whole 16-cell groups) as int32 in
//      its own LDS array, lv[PAD + c - c0] for cell c.  A lane loads 16 bytes (16 u8 or 4 f32 cells) and turns them into
//      levels; there is no prefix scan.  A cell outside the row gets the level OUTSIDE = 2^29, which no threshold reaches:
//      a threshold is x - offset <= 2^20 + 2^20.  So the count loop clamps no index and knows nothing of the row's ends.
//   2. decides its 1024 cells in 16 steps of 64 consecutive columns: lane l takes column c0 + 64 j + l at step j, reads its
//      own level, and counts the training cells below x - offset: T reads at k-G-T+i and T at k+G+1+i, every one 64
//      consecutive dwords across the wave -- 32 lanes of a bank group on 32 banks whatever G and T are -- then one
//      v_med3_i32 each and one v_add3_u32 per two (the median of level, t - 1 and t is t - 1 below t and t otherwise, so
//      the sum of the 2T medians is 2T t - count).  2T compares per cell is the work; it cannot be made independent of T
//      the way a sum can.
//   3. the 64 decisions of a step are one ballot: its population count is the step's share of the row's hits, the lane keeps
//      its own bit in a register counter of column 64 j + l (the same 16 columns over all rows of the run), and lane m keeps
//      the 16 bits of columns 16 m .. 16 m + 15, which it spreads into 16 mask bytes and stores at once.
// At the end of the run the four waves add their column counters in LDS and the workgroup issues one u32 global atomic per
// non-zero column; a row's hits are one atomic per row and tile on row_hits, which the launch zeroes first.  The level
// array is a wave's own, so the four waves meet only at the kernel's first and last barrier, and a wave loads the 16-byte
// groups of its next row before it decides the current one.
//
// fsea_cfar_shared.h has what this file shares with fsea_cfar.hip as code: the geometry's constants, level_at, spread4,
// wave_sync, the kernels' one signature, the object, its launch and the entry points.  Step 3 and the end of the run are
// fsea_cfar's as text: moved into functions they compile to other registers there ("What the detectors share").
//
// The _narrow kernels are the same code with every cell loaded on its own (any pitch and base).  In the 16-byte kernels a
// group that would begin before the row or end past its width is loaded cell by cell too, so no load leaves the row; the
// mask is written 16 bytes per lane where the width is a multiple of 16 and byte by byte otherwise.
#include "fsea_cfar_shared.h"

using fsea_detail::cfar_level_f32;
using fsea_detail::fail;
using fsea_detail::level_at;
using fsea_detail::run_of_workgroup;
using fsea_detail::spread4;
using fsea_detail::wave_sync;

namespace {

constexpr int OS_WAVES = fsea_detail::DET_WAVES;
constexpr int OS_C = fsea_detail::DET_C;          // columns per tile
constexpr int OS_PAD = (FSEA_CFAR_MAX_GUARD + FSEA_CFAR_MAX_TRAIN + 15) & ~15;   // cells of a halo at most, whole groups
constexpr int OS_SEG = OS_C + 2 * OS_PAD;         // dwords of a wave's level array
constexpr int OS_OUTSIDE = 1 << 29;               // the level of a cell outside the row: below no threshold
static_assert((OS_WAVES * OS_SEG + OS_C) * 4 <= 80 * 1024, "two workgroups per CU");
static_assert(OS_OUTSIDE > 2 * fsea_detail::CFAR_LEVEL_LIMIT + 255 && FSEA_CFAR_MAX_OFFSET == fsea_detail::CFAR_LEVEL_LIMIT,
              "x - offset stays below OUTSIDE, and OUTSIDE - (x - offset) inside an int");

struct Settings {
    int guard = 2, train = 16, offset = 60, rank = 24;
};

// Whether the group that starts at `cell` is read with one 16-byte load: the kernel may (VEC) and the group lies inside the row.
template <bool VEC, int EPG>
__device__ __forceinline__ bool whole_group(int cell, int width) {
    return VEC && cell >= 0 && cell + EPG <= width;
}

// The EPG levels of the group that starts at cell `cell` (which may lie before the row) of the row at element offset `at`:
// from `w`, its 16 bytes loaded ahead, where whole_group() holds; cell by cell inside the row otherwise; OUTSIDE outside it.
template <bool F32, bool VEC, int EPG>
__device__ __forceinline__ void levels_of(const void *__restrict__ rows, size_t at, int cell, int width, uint4 w, int (&lv)[EPG]) {
    if (whole_group<VEC, EPG>(cell, width)) {
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < EPG; ++e) {
            if (F32) lv[e] = cfar_level_f32(__uint_as_float(ws[e & 3]));
            else lv[e] = (int)((ws[e >> 2] >> (8 * (e & 3))) & 0xffu);
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < EPG; ++e) {
        const int c = cell + e;
        lv[e] = c >= 0 && c < width ? level_at<F32>(rows, at + (size_t)c) : OS_OUTSIDE;
    }
}

// the median of three: a clamped to [lo, hi] for lo <= hi, in one instruction
__device__ __forceinline__ int med3(int a, int lo, int hi) {
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(lo), "v"(hi));
    return r;
}

template <bool F32, bool VEC>
__device__ __forceinline__ void oscfar_body(const void *__restrict__ rows, size_t n_rows, size_t pitch, int width, Settings st,
                                            uint8_t *__restrict__ mask, int mask_vec, uint32_t *__restrict__ row_hits,
                                            uint32_t *__restrict__ hits) {
    constexpr int EPG = F32 ? 4 : 16;             // elements per 16-byte group
    __shared__ __attribute__((aligned(16))) int32_t lv_all[OS_WAVES][OS_SEG];
    __shared__ uint32_t total[OS_C];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t *lv = lv_all[wave];
    const int c0 = (int)blockIdx.y * OS_C;
    const int G = st.guard, T = st.train;
    const int halo = (G + T + 15) & ~15;          // <= OS_PAD
    const int g0 = c0 - halo;                     // the first staged cell: a multiple of 16, before the row in the first tile
    const int ngrp = (OS_C + 2 * halo) / EPG;     // the groups of the staged cells [g0, c0 + C + halo)
    int32_t *seg = lv + (OS_PAD - halo);          // seg[i]: the level of cell g0 + i
    size_t row0;
    const int run = run_of_workgroup<fsea_detail::DET_RUN>(n_rows, &row0);

    for (int i = tid; i < OS_C; i += fsea_detail::DET_WG) total[i] = 0u;
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};           // the lane's 16 columns, a byte each: at most DET_RUN / 4 hits
    __syncthreads();

    // the 16-byte groups of a row are loaded one row ahead: raw[c] is the lane's group of chunk c (zero where there is none)
    constexpr int NCH = (OS_SEG / EPG + 63) / 64;
    uint4 raw[NCH];
    auto fetch = [&](int rr) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int g = c * 64 + lane, cell = g0 + g * EPG;
            raw[c] = uint4{0u, 0u, 0u, 0u};
            if (rr < run && g < ngrp && whole_group<VEC, EPG>(cell, width)) {
                raw[c] = *reinterpret_cast<const uint4 *>(static_cast<const char *>(rows) +
                                                          ((row0 + rr) * pitch + (size_t)cell) * (F32 ? 4 : 1));
            }
        }
    };
    fetch(wave);

    const int two_t = 2 * T;
    for (int rr = wave; rr < run; rr += OS_WAVES) {            // the same for all lanes of a wave
        const size_t row = row0 + rr;

        // 1. the levels of the staged cells
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int g = c * 64 + lane;
            if (g < ngrp) {
                int l[EPG];
                levels_of<F32, VEC, EPG>(rows, row * pitch, g0 + g * EPG, width, raw[c], l);
                int4 *dst = reinterpret_cast<int4 *>(seg + g * EPG);
#pragma unroll
                for (int e = 0; e < EPG; e += 4) dst[e >> 2] = int4{l[e], l[e + 1], l[e + 2], l[e + 3]};
            }
        }
        fetch(rr + OS_WAVES);                                  // the next row's loads fly while this one is decided
        wave_sync();

        // 2. the decisions: column c0 + 64 j + lane at step j.  No index is clamped: the cells outside the row are in the
        // array with a level below no threshold, so the two streams are ck + a fixed offset + 64 j + i.
        const int32_t *ck = lv + OS_PAD + lane;                // ck[i]: the level of cell c0 + lane + i
        const int own = lane >> 2;                             // the step whose ballot holds the lane's 16 mask bits
        uint32_t mybits = 0u, rh = 0u;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                const int j = 4 * jj + q, kk = 64 * j + lane, k = c0 + kk;
                const int t = ck[64 * j] - st.offset;          // a training cell counts when its level is below t
                const int32_t *left = ck + 64 * j - G - T, *right = ck + 64 * j + G + 1;
                // med3(a, t - 1, t) is t - 1 for a level below t and t otherwise: the 2T of them add up to 2T t - count, at
                // one v_med3_i32 per compare and one v_add3_u32 per two (a compare, a select and an add with carry were 2
                // vector instructions per compare).  u32 sums: 2T |t| <= 2^9 (2^21 + 255) for a cell inside the row, and
                // what a cell outside it (t = OUTSIDE - offset) gives is not used.
                const int t1 = t - 1;
                uint32_t sum = 0u;
                int i = 0;
                for (; i + 8 <= T; i += 8) {                   // eight cells of each side at a time, then what is left of T
#pragma unroll
                    for (int u = 0; u < 8; ++u) sum += (uint32_t)med3(left[i + u], t1, t) + (uint32_t)med3(right[i + u], t1, t);
                }
                for (; i < T; ++i) sum += (uint32_t)med3(left[i], t1, t) + (uint32_t)med3(right[i], t1, t);
                const uint32_t below = (uint32_t)two_t * (uint32_t)t - sum;
                const int n = min(max(k - G, 0), T) + min(max(width - 1 - k - G, 0), T);   // the cells inside the row
                // count >= ceil(R n / 2T), without the division; n == 0: no hit
                const bool hit = k < width && n > 0 && below * (uint32_t)two_t >= (uint32_t)(st.rank * n);
                if (mask && !mask_vec && k < width) mask[row * (size_t)width + k] = hit ? 255 : 0;
                const unsigned long long b = __ballot(hit);
                rh += (uint32_t)__popcll(b);
                cnt[jj] += (hit ? 1u : 0u) << (8 * q);
                if (own == j) mybits = (uint32_t)(b >> (16 * (lane & 3))) & 0xffffu;
            }
        }
        const int col = c0 + 16 * lane;
        if (mask && mask_vec && col < width) {                 // width is a multiple of 16: the group is inside
            *reinterpret_cast<uint4 *>(mask + row * (size_t)width + col) =
                uint4{spread4(mybits), spread4(mybits >> 4), spread4(mybits >> 8), spread4(mybits >> 12)};
        }
        if (row_hits && lane == 0 && rh) atomicAdd(&row_hits[row], rh);
        wave_sync();                                           // before the next row overwrites lv
    }

    // 3. the run's column hits: the four waves in LDS, then one global atomic per non-zero column
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t n = (cnt[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (n) atomicAdd(&total[64 * j + lane], n);
    }
    __syncthreads();
    for (int i = tid; i < OS_C; i += fsea_detail::DET_WG) {
        const uint32_t v = total[i];
        if (v && c0 + i < width) atomicAdd(&hits[c0 + i], v);
    }
}

}  // namespace

FSEA_DETECTOR_KERNEL(fsea_oscfar_u8, oscfar_body, 4, false, true)
FSEA_DETECTOR_KERNEL(fsea_oscfar_f32, oscfar_body, 4, true, true)
FSEA_DETECTOR_KERNEL(fsea_oscfar_u8_narrow, oscfar_body, 4, false, false)
FSEA_DETECTOR_KERNEL(fsea_oscfar_f32_narrow, oscfar_body, 4, true, false)

// object, launch and entry points: fsea_cfar_shared.h
struct fsea_oscfar : fsea_detail::Detector<Settings, fsea_oscfar_u8, fsea_oscfar_f32, fsea_oscfar_u8_narrow, fsea_oscfar_f32_narrow> {};

extern "C" {

int fsea_oscfar_create(fsea_oscfar **out, int width, int device) {
    return fsea_detail::detector_create(out, width, device, "oscfar", "fsea_oscfar_create");
}

int fsea_oscfar_destroy(fsea_oscfar *c) { return fsea_detail::destroy_object(c); }

int fsea_oscfar_reset(fsea_oscfar *c) { return fsea_detail::detector_reset(c, "oscfar is NULL"); }

int fsea_oscfar_set(fsea_oscfar *c, int guard, int train, int offset, int rank) {
    if (int rc = fsea_detail::detector_check_set(c, "oscfar", guard, train, offset)) return rc;
    if (rank < 1 || rank > 2 * train) return fail(FSEA_EINVAL, "rank must be in [1, 2 * train = %d], got %d", 2 * train, rank);
    std::lock_guard<std::mutex> lock(c->mu);
    c->set = Settings{guard, train, offset, rank};
    return FSEA_OK;
}

int fsea_oscfar_width(const fsea_oscfar *c) { return c ? c->width : 0; }

uint64_t fsea_oscfar_rows(const fsea_oscfar *c) { return c ? c->rows : 0; }

int fsea_oscfar_rank(const fsea_oscfar *c) { return c ? c->set.rank : 0; }

int fsea_oscfar_add_device(fsea_oscfar *c, const void *d_rows, int type, size_t n_rows, size_t pitch, uint8_t *d_mask,
                           uint32_t *d_row_hits, void *stream) {
    return fsea_detail::detector_add_device(c, "oscfar", d_rows, type, n_rows, pitch, d_mask, d_row_hits, stream);
}

int fsea_oscfar_add_host(fsea_oscfar *c, const void *rows, int type, size_t n_rows, size_t pitch, uint8_t *mask, uint32_t *row_hits) {
    return fsea_detail::detector_add_host(c, "oscfar", rows, type, n_rows, pitch, mask, row_hits);
}

int fsea_oscfar_hits_host(fsea_oscfar *c, uint32_t *hits) { return fsea_detail::detector_hits_host(c, "oscfar", hits); }

}  // extern "C"
