// fsea_tcfar.hip -- the time-axis CFAR detector (include/fsea.h: fsea_tcfar_*): fsea_cfar's question put down each column.
// A cell is compared with the mean level of the cells of its own column in the rows before and after it, so an emission
// wider than any frequency window but short in time stands out.  Integer and order-free like fsea_cfar: every mask byte, row
// count and hit count is the same whatever the launch geometry or the cut of the rows into calls, given the context rows.
//
// Kernels fsea_tcfar_u8 / fsea_tcfar_f32 (and their _narrow forms; DESIGN.md section 4, "The time-axis CFAR detector"): a
// workgroup is one wave of 64 lanes; it owns a tile of FSEA_TCFAR_TILE_COLUMNS = 1024 columns and a run of
// FSEA_TCFAR_RUN_ROWS = 32 decided rows.  A lane owns 16 consecutive columns (one 16-byte group of u8 cells, four of f32
// cells) and keeps their two window sums SL and SR in registers, int32 and exact.  Columns never talk to one another: the
// kernel has no LDS and no barrier.
//   1. prologue: the sums of the run's first row, the T rows of each window added up one by one (2T row reads at most, each
//      independent of the others), clipped to the rows of the call.
//   2. per decided row r five row reads, every one 16 bytes per lane and coalesced along the row: the cell's own row r, and
//      the rows that move the windows on to r + 1: r - G enters SL and r - G - T leaves it, r + G + T + 1 enters SR and
//      r + G + 1 leaves it.  A row outside the call is not read: its index is clamped into the call (a row that exists) and
//      its levels are taken as 0, so the loads carry no branch and the five of four rows (u8; two of f32) are in flight
//      while a row is decided.  The counts nL and nR depend on the row alone: scalar arithmetic.
//   3. the 16 decisions of a lane are 16 bits; with FSEA_TCFAR_MASK_OR / _AND the 16 mask bytes already there are read and
//      combined; the bits are spread into 16 mask bytes stored at once, added to the lane's 16 column counters (a byte
//      each, 32 rows at most) and their population count, summed over the wave, is the row's one atomic on row_hits.
// At the end of the run a lane issues one u32 global atomic per non-zero column.
//
// The cost per cell does not depend on T; a run pays its prologue once, 2T row reads beside the 5 x 32 of its rows.
//
// The _narrow kernels are the same code with every cell loaded on its own (any pitch and base).  In the 16-byte kernels a
// group that would end past the row's width is loaded cell by cell too, so no load passes the width; the mask is read and
// written 16 bytes per lane where the width is a multiple of 16 and byte by byte otherwise.
#include "fsea_cfar_shared.h"

#include <algorithm>
#include <type_traits>

using fsea_detail::DeviceGuard;
using fsea_detail::cfar_level_f32;
using fsea_detail::fail;
using fsea_detail::level_at;
using fsea_detail::run_of_workgroup;
using fsea_detail::spread4;

namespace {

constexpr int TC_WG = 64;                         // lanes per workgroup: one wave
constexpr int TC_CPL = 16;                        // columns per lane
constexpr int TC_C = FSEA_TCFAR_TILE_COLUMNS;     // columns per tile
constexpr int TC_RUN = FSEA_TCFAR_RUN_ROWS;       // decided rows per workgroup
static_assert(TC_C == TC_WG * TC_CPL, "a lane owns 16 columns and stores 16 mask bytes");
static_assert(TC_RUN <= 255, "a lane counts a column in a byte");

struct Settings {
    int guard = 2, train = 16, offset = 60, method = FSEA_CFAR_CA, op = FSEA_TCFAR_MASK_SET;
};

// The 16-byte groups of a lane's 16 cells of one row: one of u8 cells, four of f32 cells.
template <bool F32>
struct Raw {
    uint4 g[F32 ? 4 : 1];
};

// One lane's view of the rows of a call: rows lo .. hi exist (lo <= 0 <= hi), the lane's cells are columns col .. col + 15.
template <bool F32, bool VEC>
struct Column {
    using Cell = std::conditional_t<F32, float, uint8_t>;
    static constexpr int EPG = F32 ? 4 : 16, NG = TC_CPL / EPG;
    const Cell *rows;
    ptrdiff_t pitch, lo, hi;
    int col, width;

    // whether group g is read with one 16-byte load: the kernel may (VEC) and the group ends inside the width
    __device__ __forceinline__ bool whole(int g) const { return VEC && col + (g + 1) * EPG <= width; }

    // The whole groups of row r, or of the nearest row of the call where r is outside it (levels() drops those).
    __device__ __forceinline__ void fetch(ptrdiff_t r, Raw<F32> &w) const {
        const Cell *p = rows + std::min(std::max(r, lo), hi) * pitch + col;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            w.g[g] = uint4{0u, 0u, 0u, 0u};
            if (whole(g)) w.g[g] = *reinterpret_cast<const uint4 *>(p + g * EPG);
        }
    }

    // The 16 levels of row r: from `w`, fetched ahead, where whole() holds; cell by cell below the width otherwise; 0 for a
    // cell past the width or a row outside the call.
    __device__ __forceinline__ void levels(ptrdiff_t r, const Raw<F32> &w, int (&lv)[TC_CPL]) const {
        const bool exists = r >= lo && r <= hi;
        const Cell *p = rows + (exists ? r : 0) * pitch;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const uint32_t ws[4] = {w.g[g].x, w.g[g].y, w.g[g].z, w.g[g].w};
#pragma unroll
            for (int e = 0; e < EPG; ++e) {
                const int c = col + g * EPG + e;
                int v;
                if (whole(g)) v = F32 ? cfar_level_f32(__uint_as_float(ws[e & 3])) : (int)((ws[e >> 2] >> (8 * (e & 3))) & 0xffu);
                else v = exists && c < width ? level_at<F32>(p, (size_t)c) : 0;
                lv[g * EPG + e] = exists ? v : 0;
            }
        }
    }
};

// bit e: byte e of the 16 bytes is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint4 m) {
    const uint32_t ws[4] = {m.x, m.y, m.z, m.w};
    uint32_t bits = 0u;
#pragma unroll
    for (int e = 0; e < TC_CPL; ++e) bits |= (uint32_t)(((ws[e >> 2] >> (8 * (e & 3))) & 0xffu) != 0u) << e;
    return bits;
}

template <bool F32, bool VEC>
__device__ __forceinline__ void tcfar_body(const void *__restrict__ rows, size_t n_rows, size_t pitch, int width, Settings st,
                                           int before, int after, uint8_t *__restrict__ mask, int mask_vec,
                                           uint32_t *__restrict__ row_hits, uint32_t *__restrict__ hits) {
    const int lane = threadIdx.x;
    const int G = st.guard, T = st.train;
    size_t row0;
    const int run = run_of_workgroup<TC_RUN>(n_rows, &row0);
    const Column<F32, VEC> in{static_cast<const typename Column<F32, VEC>::Cell *>(rows), (ptrdiff_t)pitch, -(ptrdiff_t)before,
                              (ptrdiff_t)n_rows + after - 1, (int)blockIdx.y * TC_C + TC_CPL * lane, width};
    const int col = in.col;
    uint32_t valid = 0u;                              // bit e: column col + e is inside the width
#pragma unroll
    for (int e = 0; e < TC_CPL; ++e) valid |= (uint32_t)(col + e < width) << e;

    // 1. the window sums of the run's first row
    int SL[TC_CPL], SR[TC_CPL], lv[TC_CPL];
#pragma unroll
    for (int e = 0; e < TC_CPL; ++e) SL[e] = SR[e] = 0;
    ptrdiff_t r = (ptrdiff_t)row0;
    Raw<F32> w;
#pragma unroll 8
    for (ptrdiff_t i = std::max(r - G - T, in.lo); i <= std::min(r - G - 1, in.hi); ++i) {
        in.fetch(i, w);
        in.levels(i, w, lv);
#pragma unroll
        for (int e = 0; e < TC_CPL; ++e) SL[e] += lv[e];
    }
#pragma unroll 8
    for (ptrdiff_t i = std::max(r + G + 1, in.lo); i <= std::min(r + G + T, in.hi); ++i) {
        in.fetch(i, w);
        in.levels(i, w, lv);
#pragma unroll
        for (int e = 0; e < TC_CPL; ++e) SR[e] += lv[e];
    }

    // 2. the rows of the run; the five reads of a row are issued DEPTH rows ahead, into the ring slot of the row just decided
    const int is_ca = -(int)(st.method == FSEA_CFAR_CA), is_go = -(int)(st.method == FSEA_CFAR_GO), is_so = ~(is_ca | is_go);
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};               // the lane's 16 columns, a byte each: at most TC_RUN hits
    struct Five {
        Raw<F32> x, a, b, c, d;
    };
    constexpr int DEPTH = F32 ? 2 : 4;                // rows in flight: 20 (u8) or 80 (f32) registers each
    Five ring[DEPTH];
    auto fetch5 = [&](ptrdiff_t q, Five &f) {         // clamped into the call: behind the run's last row they are not used
        in.fetch(q, f.x);
        in.fetch(q - G, f.a);
        in.fetch(q - G - T, f.b);
        in.fetch(q + G + T + 1, f.c);
        in.fetch(q + G + 1, f.d);
    };
    auto decide_row = [&](int rr, const Five &f) {
        const int nL = (int)std::max<ptrdiff_t>(0, std::min(r - G - 1, in.hi) - std::max(r - G - T, in.lo) + 1);
        const int nR = (int)std::max<ptrdiff_t>(0, std::min(r + G + T, in.hi) - std::max(r + G + 1, in.lo) + 1);
        const int oL = st.offset * nL, oR = st.offset * nR;
        in.levels(r, f.x, lv);
        uint32_t bits = 0u;
#pragma unroll
        for (int e = 0; e < TC_CPL; ++e) {
            const int dL = lv[e] * nL - SL[e] - oL, dR = lv[e] * nR - SR[e] - oR;   // 0 for an empty side
            // GO: an empty side (d = 0) stands back for the other; both empty: 0, no hit
            const int gL = nL == 0 ? dR : dL, gR = nR == 0 ? dL : dR;
            const int v = ((dL + dR) & is_ca) | (min(gL, gR) & is_go) | (max(dL, dR) & is_so);
            bits |= (uint32_t)(v > 0) << e;
        }
        uint8_t *m = mask ? mask + (row0 + rr) * (size_t)width + col : nullptr;
        if (st.op != FSEA_TCFAR_MASK_SET) {           // the bytes already there: any non-zero byte counts as set
            uint32_t old = 0u;
            if (mask_vec) {
                if (valid) old = nonzero_bytes(*reinterpret_cast<const uint4 *>(m));
            } else {
#pragma unroll
                for (int e = 0; e < TC_CPL; ++e) {
                    if (valid >> e & 1u) old |= (uint32_t)(m[e] != 0) << e;
                }
            }
            bits = st.op == FSEA_TCFAR_MASK_OR ? bits | old : bits & old;
        }
        bits &= valid;
        if (m) {
            if (mask_vec) {                           // width is a multiple of 16: the group is inside or outside
                if (valid) *reinterpret_cast<uint4 *>(m) = uint4{spread4(bits), spread4(bits >> 4), spread4(bits >> 8), spread4(bits >> 12)};
            } else {
#pragma unroll
                for (int e = 0; e < TC_CPL; ++e) {
                    if (valid >> e & 1u) m[e] = bits >> e & 1u ? 255 : 0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] += spread4(bits >> (4 * k)) & 0x01010101u;
        if (row_hits) {
            uint32_t n = (uint32_t)__popc(bits);
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) n += __shfl_xor(n, s);
            if (lane == 0 && n) atomicAdd(&row_hits[row0 + rr], n);
        }
        // the windows of row r + 1
        in.levels(r - G, f.a, lv);
#pragma unroll
        for (int e = 0; e < TC_CPL; ++e) SL[e] += lv[e];
        in.levels(r - G - T, f.b, lv);
#pragma unroll
        for (int e = 0; e < TC_CPL; ++e) SL[e] -= lv[e];
        in.levels(r + G + T + 1, f.c, lv);
#pragma unroll
        for (int e = 0; e < TC_CPL; ++e) SR[e] += lv[e];
        in.levels(r + G + 1, f.d, lv);
#pragma unroll
        for (int e = 0; e < TC_CPL; ++e) SR[e] -= lv[e];
    };
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) fetch5(r + k, ring[k]);
    for (int rr = 0; rr < run; rr += DEPTH) {
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            if (rr + k < run) {
                decide_row(rr + k, ring[k]);
                fetch5(r + DEPTH, ring[k]);
                ++r;
            }
        }
    }

    // 3. the run's column hits: one global atomic per non-zero column
#pragma unroll
    for (int e = 0; e < TC_CPL; ++e) {
        const uint32_t n = (cnt[e >> 2] >> (8 * (e & 3))) & 0xffu;
        if (n) atomicAdd(&hits[col + e], n);          // n counts written bits: inside the width
    }
}

}  // namespace

// A kernel `name` around tcfar_body<F32, VEC>, WAVES waves to a SIMD's registers
#define FSEA_TCFAR_KERNEL(name, WAVES, F32, VEC)                                                                              \
    extern "C" __global__ __launch_bounds__(TC_WG, WAVES) void name(                                                          \
        const void *__restrict__ rows, size_t n_rows, size_t pitch, int width, int guard, int train, int offset, int method,  \
        int op, int before, int after, uint8_t *__restrict__ mask, int mask_vec, uint32_t *__restrict__ row_hits,             \
        uint32_t *__restrict__ hits) {                                                                                        \
        tcfar_body<F32, VEC>(rows, n_rows, pitch, width, Settings{guard, train, offset, method, op}, before, after, mask,     \
                             mask_vec, row_hits, hits);                                                                       \
    }

FSEA_TCFAR_KERNEL(fsea_tcfar_u8, 2, false, true)
FSEA_TCFAR_KERNEL(fsea_tcfar_f32, 1, true, true)
FSEA_TCFAR_KERNEL(fsea_tcfar_u8_narrow, 2, false, false)
FSEA_TCFAR_KERNEL(fsea_tcfar_f32_narrow, 2, true, false)

// The object: fsea_cfar's (fsea_cfar_shared.h: create, reset, the checks of set, hits_host) with a fifth setting and a
// launch of its own, which takes the context rows.
struct fsea_tcfar : fsea_detail::RowObject {
    Settings set;                                 // at offset 16 for the fake objects of the tests
    fsea_detail::ZeroedScratch hits;              // width u32; its event orders the calls
    std::mutex mu;
    fsea_detail::HostStaging staging;             // the host forms

    // One add on device rows, asynchronous on `s`; `before` and `after` are at most G + T.  The caller holds mu, is on the
    // device and has checked the arguments.
    int add_launch(const void *d_rows, int type, size_t n_rows, size_t pitch, int before, int after, uint8_t *d_mask,
                   uint32_t *d_row_hits, hipStream_t s) {
        int rc = hits.acquire(s);
        if (rc) return rc;
        if (d_row_hits) FSEA_HIP(hipMemsetAsync(d_row_hits, 0, n_rows * sizeof(uint32_t), s));   // set, not added to
        const dim3 grid((unsigned)((n_rows + TC_RUN - 1) / TC_RUN), (unsigned)((width + TC_C - 1) / TC_C));
        const bool vec = fsea_detail::rows_vec16(d_rows, pitch * fsea_detail::row_elem_bytes(type));
        const int mask_vec = width % 16 == 0;
        const auto kernel = type == FSEA_CFAR_U8 ? (vec ? fsea_tcfar_u8 : fsea_tcfar_u8_narrow) : (vec ? fsea_tcfar_f32 : fsea_tcfar_f32_narrow);
        hipLaunchKernelGGL(kernel, grid, dim3(TC_WG), 0, s, d_rows, n_rows, pitch, width, set.guard, set.train, set.offset,
                           set.method, set.op, before, after, d_mask, mask_vec, d_row_hits, static_cast<uint32_t *>(hits.buf.ptr));
        FSEA_HIP(hipGetLastError());
        rows += n_rows;
        return hits.release(s);
    }
};

namespace {

// What both add forms check before any device work, in the header's order up to the span; the device form goes on with the
// alignment.  The three row counts are added without overflow: a count above the span's limit is refused by the span.
int check_add(const fsea_tcfar *t, const void *rows, int type, size_t n_rows, size_t pitch, size_t rows_before, size_t rows_after) {
    if (!t) return fail(FSEA_EINVAL, "tcfar is NULL");
    if (int rc = fsea_detail::check_rows_head("row", type, n_rows)) return rc;
    if (n_rows == 0) return FSEA_OK;
    const size_t all = n_rows + std::min(rows_before, fsea_detail::ROWS_MAX_SPAN) + std::min(rows_after, fsea_detail::ROWS_MAX_SPAN);
    return fsea_detail::check_rows_planes(t->width, all, "", fsea_detail::RowPlane{rows, "pitch", pitch});
}

int check_op_has_mask(const Settings &set, const uint8_t *mask) {
    if (set.op != FSEA_TCFAR_MASK_SET && !mask) return fail(FSEA_EINVAL, "mask operation %d combines with a mask, and the mask is NULL", set.op);
    return FSEA_OK;
}

}  // namespace

extern "C" {

int fsea_tcfar_create(fsea_tcfar **out, int width, int device) {
    return fsea_detail::detector_create(out, width, device, "tcfar", "fsea_tcfar_create");
}

int fsea_tcfar_destroy(fsea_tcfar *t) { return fsea_detail::destroy_object(t); }

int fsea_tcfar_reset(fsea_tcfar *t) { return fsea_detail::detector_reset(t, "tcfar is NULL"); }

int fsea_tcfar_set(fsea_tcfar *t, int guard, int train, int offset, int method, int mask_op) {
    if (int rc = fsea_detail::detector_check_set(t, "tcfar", guard, train, offset)) return rc;
    if (method != FSEA_CFAR_CA && method != FSEA_CFAR_GO && method != FSEA_CFAR_SO) return fail(FSEA_EINVAL, "unknown method %d", method);
    if (mask_op != FSEA_TCFAR_MASK_SET && mask_op != FSEA_TCFAR_MASK_OR && mask_op != FSEA_TCFAR_MASK_AND) {
        return fail(FSEA_EINVAL, "unknown mask operation %d", mask_op);
    }
    std::lock_guard<std::mutex> lock(t->mu);
    t->set = Settings{guard, train, offset, method, mask_op};
    return FSEA_OK;
}

int fsea_tcfar_width(const fsea_tcfar *t) { return t ? t->width : 0; }

uint64_t fsea_tcfar_rows(const fsea_tcfar *t) { return t ? t->rows : 0; }

int fsea_tcfar_run_rows(const fsea_tcfar *t) { return t ? TC_RUN : 0; }

int fsea_tcfar_add_device(fsea_tcfar *t, const void *d_rows, int type, size_t n_rows, size_t pitch, size_t rows_before,
                          size_t rows_after, uint8_t *d_mask, uint32_t *d_row_hits, void *stream) {
    int rc = check_add(t, d_rows, type, n_rows, pitch, rows_before, rows_after);
    if (!rc && n_rows) rc = fsea_detail::check_aligned16("d_rows, d_mask and d_row_hits", d_rows, d_mask, d_row_hits);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(t->mu);
    if ((rc = check_op_has_mask(t->set, d_mask))) return rc;
    if ((rc = fsea_detail::check_rows_room(t, n_rows))) return rc;
    FSEA_ON_DEVICE(t->device);
    const size_t reach = (size_t)(t->set.guard + t->set.train);   // context beyond G + T rows is never read
    return t->add_launch(d_rows, type, n_rows, pitch, (int)std::min(rows_before, reach), (int)std::min(rows_after, reach), d_mask,
                         d_row_hits, static_cast<hipStream_t>(stream));
}

int fsea_tcfar_add_host(fsea_tcfar *t, const void *rows, int type, size_t n_rows, size_t pitch, size_t rows_before,
                        size_t rows_after, uint8_t *mask, uint32_t *row_hits) {
    int rc = check_add(t, rows, type, n_rows, pitch, rows_before, rows_after);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(t->mu);
    if ((rc = check_op_has_mask(t->set, mask))) return rc;
    if ((rc = fsea_detail::check_rows_room(t, n_rows))) return rc;
    // The rows go up packed, in chunks: the decided rows of a chunk between their context rows, at most G + T each side,
    // taken from the caller's array; where the operation reads the mask, the chunk's mask bytes behind them.
    const size_t width = (size_t)t->width, esz = fsea_detail::row_elem_bytes(type);
    const fsea_detail::PackedPlane in(rows, pitch * esz, width * esz);
    const size_t reach = (size_t)(t->set.guard + t->set.train), room = fsea_detail::ROWS_STAGE_BYTES / in.packed;
    if (room < 2 * reach + 1) {
        return fail(FSEA_EINVAL, "rows of %zu bytes: the %zu rows of one decided row and its context do not fit the staging of %zu bytes; "
                                 "use fsea_tcfar_add_device", in.packed, 2 * reach + 1, fsea_detail::ROWS_STAGE_BYTES);
    }
    const bool reads_mask = t->set.op != FSEA_TCFAR_MASK_SET;
    const size_t chunk = room - 2 * reach;
    FSEA_ON_DEVICE(t->device);
    const char *first = static_cast<const char *>(rows) - (ptrdiff_t)(std::min(rows_before, reach) * pitch * esz);
    const fsea_detail::PackedPlane all(first, pitch * esz, width * esz);   // row 0: the first row a chunk may take
    const size_t lead = std::min(rows_before, reach), tail = std::min(rows_after, reach);
    for (size_t r0 = 0; r0 < n_rows; r0 += chunk) {
        const size_t nr = std::min(chunk, n_rows - r0);
        const size_t b = std::min(r0 + lead, reach), a = std::min(n_rows - r0 - nr + tail, reach);
        const size_t row_bytes = (b + nr + a) * in.packed, mask_bytes = reads_mask ? nr * width : 0;
        const fsea_detail::HostStaging::Part parts[2] = {{mask ? mask + r0 * width : nullptr, nr * width},
                                                         {row_hits ? row_hits + r0 : nullptr, nr * sizeof(uint32_t)}};
        rc = t->staging.run(
            row_bytes + mask_bytes, parts,
            [&](void *h_in) {
                all.pack(h_in, r0 + lead - b, b + nr + a);
                if (mask_bytes) std::memcpy(static_cast<char *>(h_in) + row_bytes, mask + r0 * width, mask_bytes);
            },
            [&](void *d_in, void **d_parts, hipStream_t s) -> int {
                char *d = static_cast<char *>(d_in);
                if (mask_bytes) FSEA_HIP(hipMemcpyAsync(d_parts[0], d + row_bytes, mask_bytes, hipMemcpyDeviceToDevice, s));
                return t->add_launch(d + b * in.packed, type, nr, in.packed / esz, (int)b, (int)a, static_cast<uint8_t *>(d_parts[0]),
                                     static_cast<uint32_t *>(d_parts[1]), s);
            });
        if (rc) return rc;
    }
    return FSEA_OK;
}

int fsea_tcfar_hits_host(fsea_tcfar *t, uint32_t *hits) { return fsea_detail::detector_hits_host(t, "tcfar", hits); }

}  // extern "C"
