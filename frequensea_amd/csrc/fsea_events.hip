// fsea_events.hip -- spectrum events (include/fsea.h: fsea_events_*): a resident detection mask, and optionally the level rows
// under it, reduced to a sorted list of runs (a few records per row); the runs linked into time-frequency events on the host
// (fsea_events_link); the surviving runs painted back as a cleaned mask or label image.  Integer like the CFAR detector
// (fsea_cfar.hip) whose masks it reads: every record is the same bits whatever the launch geometry or the cut of the rows
// into calls.
//
// The run kernels ("Spectrum events"): one wave per row, four rows per workgroup.  A run can span any
// number of chunks, so the wave walks its row in chunks of 64 lanes x 16 cells and carries the open run from chunk to chunk.
// Per chunk a lane
//   1. turns its 16 mask bytes, loaded at once one chunk ahead, into 16 hit bits; a chunk without a hit ends here (one
//      ballot);
//   2. takes part in an inclusive max-scan of "position of the last hit" over the lanes (six __shfl_up steps); shifted by one
//      lane, with the carry in lane 0, that is the hit before the lane's first cell.  A hit starts a run iff more than G
//      non-hit columns lie between it and the hit before it, or there is none: 16 compares in registers;
//   3. (pass 2 only) loads the 16 levels if its group has a hit and sums up its trailing segment -- the hits from its last
//      start on, or all of them where it starts no run: first column, hit count, level sum, peak and peak column.  A
//      segmented scan over the lanes (a segment begins at a lane that starts a run) and the carry give every lane the open run
//      that enters it, a prefix sum of the start counts gives the run's number in the row;
//   4. (pass 2 only) walks its cells again: at every start it stores the run that ends there -- the entering one joined with
//      the lane's hits before the start, or one that began in this very lane.  The row's last run is stored from the carry.
// Two passes keep the list sorted without a global atomic or a sort: fsea_events_count writes the number of runs per row,
// fsea_events_scan_rows and fsea_events_scan_tiles turn that into each row's first index and the total, and pass 2
// (fsea_events_runs, _u8, _f32) computes the runs again and stores the records whose index is below the capacity.  A wave
// whose row begins at or beyond the capacity leaves at once.  Every loop has a bound known on entry (the chunks of a row, the
// steps of a scan, the tiles of the row counts); no wave waits for another.
//
// The _narrow kernels are the same code with every byte and level loaded on its own (any pitch and base).  In the 16-byte
// kernels a group that would end past the row's width is loaded cell by cell too, so no load passes the width.  u8 levels are
// summed in 32 bits (2^20 cells of 255), f32 levels in 64 (2^20 cells of 2^20).
//
// fsea_events_paint: one wave per run stores the run's value over first .. last of its image row, 16 bytes per lane in the
// aligned middle and single bytes at both ends, behind a zero fill of the image rows.
#include "fsea_rows.h"

#include <climits>
#include <type_traits>
#include <vector>

using fsea_detail::DeviceGuard;
using fsea_detail::cfar_level_f32;
using fsea_detail::fail;

static_assert(sizeof(fsea_events_run) == 32 && sizeof(fsea_events_event) == 48, "the records of include/fsea.h");

namespace {

constexpr int EV_WG = 256;                        // lanes per workgroup
constexpr int EV_WAVES = EV_WG / 64;              // rows (runs, for the paint) per workgroup
constexpr int EV_CHUNK = 64 * 16;                 // cells of a wave's step along its row
constexpr int EV_NONE = -(1 << 29);               // "no hit so far": far enough below column 0 for any G, no overflow
constexpr int EV_TILE = 4 * EV_WG;                // rows whose counts one workgroup of the scan adds up
static_assert(FSEA_EVENTS_MAX_GAP_COLS < EV_CHUNK && FSEA_EVENTS_MAX_WIDTH <= (1 << 20), "positions and sums stay in range");

// bit i of the result: byte i of w is not zero
__device__ __forceinline__ uint32_t nonzero4(uint32_t w) {
    const uint32_t t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

// A stretch of hits that belong to one run.  first < 0: the stretch starts no run, it continues whatever came before it.
template <class S>
struct Seg {
    int first;
    uint32_t hits;
    int peak, peak_col;
    S sum;
};

template <class S>
__device__ __forceinline__ Seg<S> seg_empty(int first) { return Seg<S>{first, 0u, INT_MIN, 0, (S)0}; }

template <int LV, class S>
__device__ __forceinline__ void seg_add(Seg<S> &t, int pos, int lv) {
    ++t.hits;
    if (LV) {
        t.sum += (S)lv;
        if (lv > t.peak) {                        // strict: the lowest column keeps a tie
            t.peak = lv;
            t.peak_col = pos;
        }
    }
}

// a, then b to its right
template <int LV, class S>
__device__ __forceinline__ Seg<S> seg_join(Seg<S> a, const Seg<S> &b) {
    if (b.first >= 0) return b;
    a.hits += b.hits;
    if (LV) {
        a.sum += b.sum;
        if (b.peak > a.peak) {
            a.peak = b.peak;
            a.peak_col = b.peak_col;
        }
    }
    return a;
}

template <int LV, class S>
__device__ __forceinline__ Seg<S> seg_shfl_up(const Seg<S> &v, int d) {
    Seg<S> u;
    u.first = __shfl_up(v.first, d);
    u.hits = __shfl_up(v.hits, d);
    u.peak = LV ? __shfl_up(v.peak, d) : INT_MIN;
    u.peak_col = LV ? __shfl_up(v.peak_col, d) : 0;
    u.sum = LV ? __shfl_up(v.sum, d) : (S)0;
    return u;
}

template <int LV, class S>
__device__ __forceinline__ Seg<S> seg_shfl(const Seg<S> &v, int src) {
    Seg<S> u;
    u.first = __shfl(v.first, src);
    u.hits = __shfl(v.hits, src);
    u.peak = LV ? __shfl(v.peak, src) : INT_MIN;
    u.peak_col = LV ? __shfl(v.peak_col, src) : 0;
    u.sum = LV ? __shfl(v.sum, src) : (S)0;
    return u;
}

// one record, where it lies below the capacity: two 16-byte stores
template <int LV, class S>
__device__ __forceinline__ void put_run(fsea_events_run *__restrict__ runs, size_t capacity, unsigned long long at, uint32_t row,
                                        const Seg<S> &t, int last) {
    if (at >= capacity) return;
    const long long sum = LV ? (long long)t.sum : 0ll;
    uint4 *dst = reinterpret_cast<uint4 *>(runs + at);
    dst[0] = uint4{row, (uint32_t)t.first, (uint32_t)last, t.hits};
    dst[1] = uint4{LV ? (uint32_t)t.peak : 0u, (uint32_t)(LV ? t.peak_col : t.first), (uint32_t)((unsigned long long)sum & 0xffffffffull),
                   (uint32_t)((unsigned long long)sum >> 32)};
}

// LV: 0 no levels, 1 u8, 2 f32.  EMIT: pass 2 (the records) or pass 1 (the row's count).
template <int LV, bool VEC, bool EMIT>
__device__ __forceinline__ void runs_body(const uint8_t *__restrict__ mask, size_t mask_pitch, const void *__restrict__ levels,
                                          size_t level_pitch, size_t n_rows, int width, int G, uint32_t row_base,
                                          uint32_t *__restrict__ counts, const unsigned long long *__restrict__ tile_base,
                                          fsea_events_run *__restrict__ runs, size_t capacity) {
    using S = std::conditional_t<LV == 2, long long, int>;
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * EV_WAVES + (threadIdx.x >> 6);
    if (r >= n_rows) return;                                   // the whole wave: every shuffle below has its 64 lanes
    unsigned long long at0 = 0;
    if (EMIT) {
        at0 = tile_base[r / EV_TILE] + counts[r];
        if (at0 >= capacity) return;                           // nothing of this row is stored
    }
    const uint32_t row = row_base + (uint32_t)r;
    const uint8_t *__restrict__ mrow = mask + r * mask_pitch;
    const size_t lrow = r * level_pitch;
    const int n_chunks = (width + EV_CHUNK - 1) / EV_CHUNK;

    int carry_last = EV_NONE;                                  // the last hit so far, the same in every lane
    int carry_cnt = 0;                                         // runs started so far (pass 1: this lane's own starts)
    Seg<S> carry = seg_empty<S>(-1);                           // the open run

    // 1. the lane's 16 hit bits; the 16 bytes of a chunk are loaded while the chunk before it is worked on (four chunks ahead
    //    measured no faster: DESIGN.md)
    uint4 ahead = uint4{0u, 0u, 0u, 0u};
    auto fetch = [&](int c) {
        const int cell = c * EV_CHUNK + lane * 16;
        if (VEC && c < n_chunks && cell + 16 <= width) ahead = *reinterpret_cast<const uint4 *>(mrow + cell);
    };
    fetch(0);
    for (int c = 0; c < n_chunks; ++c) {
        const int cell = c * EV_CHUNK + lane * 16;
        uint32_t hb = 0u;
        if (VEC && cell + 16 <= width) {
            hb = nonzero4(ahead.x) | (nonzero4(ahead.y) << 4) | (nonzero4(ahead.z) << 8) | (nonzero4(ahead.w) << 12);
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (cell + e < width && mrow[cell + e] != 0) hb |= 1u << e;
            }
        }
        fetch(c + 1);
        if (__ballot(hb != 0u) == 0ull) continue;              // wave-uniform: no hit in the chunk, the carry stands

        // 2. the hit before the lane's first cell
        const int lp = hb ? cell + 31 - __clz((int)hb) : EV_NONE;
        int sc = lp;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(sc, d);
            if (lane >= d) sc = max(sc, up);
        }
        int before = __shfl_up(sc, 1);
        before = lane == 0 ? carry_last : max(before, carry_last);
        carry_last = max(carry_last, __shfl(sc, 63));

        if (!EMIT) {
            int prev = before;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if ((hb >> e) & 1u) {
                    carry_cnt += (cell + e) - prev - 1 > G;
                    prev = cell + e;
                }
            }
            continue;
        }

        // 3. the levels under the lane's hits, its trailing segment and where its runs start
        int lv[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) lv[e] = 0;
        if (LV && hb) {
            if (VEC && cell + 16 <= width) {
                if (LV == 1) {
                    const uint4 w = *reinterpret_cast<const uint4 *>(static_cast<const uint8_t *>(levels) + lrow + cell);
                    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int e = 0; e < 16; ++e) lv[e] = (int)((ws[e >> 2] >> (8 * (e & 3))) & 0xffu);
                } else {
                    const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const float *>(levels) + lrow + cell);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint4 w = src[q];
                        lv[4 * q] = cfar_level_f32(__uint_as_float(w.x));
                        lv[4 * q + 1] = cfar_level_f32(__uint_as_float(w.y));
                        lv[4 * q + 2] = cfar_level_f32(__uint_as_float(w.z));
                        lv[4 * q + 3] = cfar_level_f32(__uint_as_float(w.w));
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if ((hb >> e) & 1u) {
                        lv[e] = LV == 1 ? (int)static_cast<const uint8_t *>(levels)[lrow + cell + e]
                                        : cfar_level_f32(static_cast<const float *>(levels)[lrow + cell + e]);
                    }
                }
            }
        }
        uint32_t starts = 0u;
        Seg<S> t = seg_empty<S>(-1);
        {
            int prev = before;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if ((hb >> e) & 1u) {
                    if ((cell + e) - prev - 1 > G) {
                        starts |= 1u << e;
                        t = seg_empty<S>(cell + e);
                    }
                    seg_add<LV>(t, cell + e, lv[e]);
                    prev = cell + e;
                }
            }
        }
        const int ns = __popc(starts);
        int cnt = ns;
        Seg<S> in = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int cu = __shfl_up(cnt, d);
            const Seg<S> u = seg_shfl_up<LV>(in, d);
            if (lane >= d) {
                cnt += cu;
                in = seg_join<LV>(u, in);
            }
        }
        const int chunk_cnt = __shfl(cnt, 63);
        const Seg<S> chunk_seg = seg_shfl<LV>(in, 63);
        Seg<S> cur = seg_shfl_up<LV>(in, 1);
        if (lane == 0) cur = seg_empty<S>(-1);
        cur = seg_join<LV>(carry, cur);                        // the run that is open where the lane's cells begin
        int idx = carry_cnt + cnt - ns - 1;                    // its number in the row; -1: none yet
        carry = seg_join<LV>(carry, chunk_seg);
        carry_cnt += chunk_cnt;

        // 4. a run ends where the next one starts
        if (starts) {
            int last = before;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if ((hb >> e) & 1u) {
                    if ((starts >> e) & 1u) {
                        if (idx >= 0) put_run<LV>(runs, capacity, at0 + (unsigned long long)idx, row, cur, last);
                        ++idx;
                        cur = seg_empty<S>(cell + e);
                    }
                    seg_add<LV>(cur, cell + e, lv[e]);
                    last = cell + e;
                }
            }
        }
    }

    if (!EMIT) {
        int total = carry_cnt;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d);
        if (lane == 0) counts[r] = (uint32_t)total;
        return;
    }
    if (lane == 0 && carry_cnt > 0) put_run<LV>(runs, capacity, at0 + (unsigned long long)(carry_cnt - 1), row, carry, carry_last);
}

// inclusive sum over the workgroup's 256 lanes; `total` is the workgroup's sum.  Two barriers.
template <class T>
__device__ __forceinline__ T block_scan(T v, T *__restrict__ wave_sums, T *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    __syncthreads();                                           // the sums of the round before are read
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    T below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) {
        if (w < wave) below += wave_sums[w];
        all += wave_sums[w];
    }
    *total = all;
    return v + below;
}

}  // namespace

#define FSEA_EVENTS_COUNT_KERNEL(name, VEC)                                                                                    \
    extern "C" __global__ __launch_bounds__(EV_WG) void name(const uint8_t *__restrict__ mask, size_t mask_pitch, size_t n_rows, \
                                                             int width, int gap, uint32_t *__restrict__ counts) {             \
        runs_body<0, VEC, false>(mask, mask_pitch, nullptr, 0, n_rows, width, gap, 0u, counts, nullptr, nullptr, 0);           \
    }
FSEA_EVENTS_COUNT_KERNEL(fsea_events_count, true)
FSEA_EVENTS_COUNT_KERNEL(fsea_events_count_narrow, false)
#undef FSEA_EVENTS_COUNT_KERNEL

#define FSEA_EVENTS_RUNS_KERNEL(name, LV, VEC)                                                                                 \
    extern "C" __global__ __launch_bounds__(EV_WG) void name(                                                                 \
        const uint8_t *__restrict__ mask, size_t mask_pitch, const void *__restrict__ levels, size_t level_pitch, size_t n_rows, \
        int width, int gap, uint32_t row_base, uint32_t *__restrict__ counts, const unsigned long long *__restrict__ tile_base, \
        fsea_events_run *__restrict__ runs, size_t capacity) {                                                                \
        runs_body<LV, VEC, true>(mask, mask_pitch, levels, level_pitch, n_rows, width, gap, row_base, counts, tile_base, runs, \
                                 capacity);                                                                                    \
    }
FSEA_EVENTS_RUNS_KERNEL(fsea_events_runs, 0, true)
FSEA_EVENTS_RUNS_KERNEL(fsea_events_runs_u8, 1, true)
FSEA_EVENTS_RUNS_KERNEL(fsea_events_runs_f32, 2, true)
FSEA_EVENTS_RUNS_KERNEL(fsea_events_runs_narrow, 0, false)
FSEA_EVENTS_RUNS_KERNEL(fsea_events_runs_u8_narrow, 1, false)
FSEA_EVENTS_RUNS_KERNEL(fsea_events_runs_f32_narrow, 2, false)
#undef FSEA_EVENTS_RUNS_KERNEL

// counts[r] <- the runs of the rows before r in r's tile of EV_TILE rows; tile_sums[t] <- the runs of tile t
extern "C" __global__ __launch_bounds__(EV_WG) void fsea_events_scan_rows(uint32_t *__restrict__ counts, size_t n_rows,
                                                                          unsigned long long *__restrict__ tile_sums) {
    __shared__ uint32_t wave_sums[EV_WAVES];
    const size_t base = (size_t)blockIdx.x * EV_TILE + (size_t)threadIdx.x * 4;
    uint32_t c[4], s = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = base + j < n_rows ? counts[base + j] : 0u;
        s += c[j];
    }
    uint32_t total;
    uint32_t at = block_scan(s, wave_sums, &total) - s;        // a tile holds at most 1024 * 2^19 runs
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j < n_rows) counts[base + j] = at;
        at += c[j];
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// One workgroup: tile_sums[t] <- the runs of the tiles before t, *total <- the runs of the call (mapped host memory: the
// count is with the host when the kernel is done, no copy behind it)
extern "C" __global__ __launch_bounds__(EV_WG) void fsea_events_scan_tiles(unsigned long long *__restrict__ tile_sums, size_t n_tiles,
                                                                           unsigned long long *__restrict__ total_out) {
    __shared__ unsigned long long wave_sums[EV_WAVES];
    unsigned long long carry = 0ull;
    for (size_t i0 = 0; i0 < n_tiles; i0 += EV_WG) {
        const size_t i = i0 + threadIdx.x;
        const unsigned long long v = i < n_tiles ? tile_sums[i] : 0ull;
        unsigned long long total;
        const unsigned long long incl = block_scan(v, wave_sums, &total);
        if (i < n_tiles) tile_sums[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// One wave per run.  A run outside the rows of the image, one with value 0 and one that does not lie inside the width are
// left out.
extern "C" __global__ __launch_bounds__(EV_WG) void fsea_events_paint(const fsea_events_run *__restrict__ runs,
                                                                      const uint8_t *__restrict__ values, size_t n_runs,
                                                                      unsigned long long row0, size_t n_rows, int width,
                                                                      uint8_t *__restrict__ image, size_t pitch) {
    const int lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * EV_WAVES + (threadIdx.x >> 6);
    if (i >= n_runs) return;
    const uint32_t v = values[i];
    if (v == 0u) return;
    const uint4 head = *reinterpret_cast<const uint4 *>(runs + i);             // row, first, last, hits
    const unsigned long long row = head.x;
    if (row < row0 || row - row0 >= (unsigned long long)n_rows) return;
    if (head.y > head.z || head.z >= (uint32_t)width) return;
    uint8_t *__restrict__ dst = image + (size_t)(row - row0) * pitch;
    const size_t a = head.y, b = (size_t)head.z + 1;                           // [a, b)
    const size_t to_16 = (size_t)(16u - (uint32_t)((uintptr_t)(dst + a) & 15u)) & 15u;
    const size_t m0 = a + to_16 < b ? a + to_16 : b;                           // the aligned middle [m0, m1)
    const size_t m1 = m0 + ((b - m0) & ~(size_t)15);
    if (a + lane < m0) dst[a + lane] = (uint8_t)v;                             // at most 15 bytes in front ...
    const uint32_t w = v * 0x01010101u;
    for (size_t o = m0 + (size_t)lane * 16; o < m1; o += EV_CHUNK) *reinterpret_cast<uint4 *>(dst + o) = uint4{w, w, w, w};
    if (m1 + lane < b) dst[m1 + lane] = (uint8_t)v;                            // ... and behind
}

// `gap` follows the common head: tests/test_events_host.py reads it from its fake object
struct fsea_events : fsea_detail::RowObject {
    int gap = 0;
    fsea_detail::SharedScratch scratch;           // the row counts and the tile sums of a call; its event orders the calls
    fsea_detail::MappedBuffer h_total;            // where a call's count arrives: the scan stores it into host memory itself
    unsigned long long *d_total = nullptr;        // its device address
    std::mutex mu;
    fsea_detail::HostStaging staging;             // the host forms
};

namespace {

int check_runs(const fsea_events *ev, const uint8_t *mask, size_t mask_pitch, const void *levels, int type, size_t level_pitch,
               size_t n_rows, const fsea_events_run *runs, size_t capacity, size_t *n_runs) {
    if (!ev) return fail(FSEA_EINVAL, "events is NULL");
    if (!n_runs) return fail(FSEA_EINVAL, "n_runs is NULL");
    if (int rc = fsea_detail::check_rows_head("level", type, n_rows)) return rc;
    if (!runs && capacity) return fail(FSEA_EINVAL, "NULL buffer for a capacity of %zu runs", capacity);
    if (n_rows == 0) return FSEA_OK;
    const fsea_detail::RowPlane m{mask, "mask pitch", mask_pitch}, l{levels, "level pitch", level_pitch};
    return fsea_detail::check_rows_planes(ev->width, n_rows, "mask ", m, &l);
}

struct RowsArgs {
    const uint8_t *mask;
    size_t mask_pitch;
    const void *levels;
    int type;
    size_t level_pitch, n_rows;
    bool vec() const {
        return fsea_detail::rows_vec16(mask, mask_pitch) &&
               (!levels || fsea_detail::rows_vec16(levels, level_pitch * fsea_detail::row_elem_bytes(type)));
    }
};

size_t n_tiles_of(size_t n_rows) { return (n_rows + EV_TILE - 1) / EV_TILE; }
size_t counts_bytes(size_t n_rows) { return (n_rows * sizeof(uint32_t) + 15) & ~(size_t)15; }

// Pass 1 and the scans on `s`, then the wait for the count.  The caller holds ev->mu, is on ev's device, has checked the
// arguments and has acquired the scratch for `s`; the scratch stays in use until runs_store or a release.
int runs_count(fsea_events *ev, const RowsArgs &a, unsigned long long *found, hipStream_t s) {
    uint32_t *counts = static_cast<uint32_t *>(ev->scratch.buf.ptr);
    unsigned long long *tiles = reinterpret_cast<unsigned long long *>(static_cast<char *>(ev->scratch.buf.ptr) + counts_bytes(a.n_rows));
    const size_t n_tiles = n_tiles_of(a.n_rows);
    const dim3 grid((unsigned)((a.n_rows + EV_WAVES - 1) / EV_WAVES));
    hipLaunchKernelGGL(a.vec() ? fsea_events_count : fsea_events_count_narrow, grid, dim3(EV_WG), 0, s, a.mask, a.mask_pitch, a.n_rows,
                       ev->width, ev->gap, counts);
    FSEA_HIP(hipGetLastError());
    hipLaunchKernelGGL(fsea_events_scan_rows, dim3((unsigned)n_tiles), dim3(EV_WG), 0, s, counts, a.n_rows, tiles);
    FSEA_HIP(hipGetLastError());
    hipLaunchKernelGGL(fsea_events_scan_tiles, dim3(1), dim3(EV_WG), 0, s, tiles, n_tiles, ev->d_total);
    FSEA_HIP(hipGetLastError());
    FSEA_HIP(hipStreamSynchronize(s));
    *found = *static_cast<volatile unsigned long long *>(ev->h_total.ptr);
    return FSEA_OK;
}

// Pass 2 on `s`, behind runs_count of the same rows: the first `capacity` records to d_runs.  Asynchronous.
int runs_store(fsea_events *ev, const RowsArgs &a, fsea_events_run *d_runs, size_t capacity, hipStream_t s) {
    uint32_t *counts = static_cast<uint32_t *>(ev->scratch.buf.ptr);
    const unsigned long long *tiles =
        reinterpret_cast<const unsigned long long *>(static_cast<char *>(ev->scratch.buf.ptr) + counts_bytes(a.n_rows));
    const dim3 grid((unsigned)((a.n_rows + EV_WAVES - 1) / EV_WAVES));
    const bool vec = a.vec();
    auto kernel = !a.levels ? (vec ? fsea_events_runs : fsea_events_runs_narrow)
                  : a.type == FSEA_CFAR_U8 ? (vec ? fsea_events_runs_u8 : fsea_events_runs_u8_narrow)
                                           : (vec ? fsea_events_runs_f32 : fsea_events_runs_f32_narrow);
    hipLaunchKernelGGL(kernel, grid, dim3(EV_WG), 0, s, a.mask, a.mask_pitch, a.levels, a.level_pitch, a.n_rows, ev->width, ev->gap,
                       (uint32_t)ev->rows, counts, tiles, d_runs, capacity);
    FSEA_HIP(hipGetLastError());
    return FSEA_OK;
}

// One call on device rows: count, store what fits, wait.  The caller holds ev->mu, is on ev's device, has checked all.
int runs_launch(fsea_events *ev, const RowsArgs &a, fsea_events_run *d_runs, size_t capacity, unsigned long long *found, hipStream_t s) {
    int rc = ev->scratch.acquire(counts_bytes(a.n_rows) + n_tiles_of(a.n_rows) * sizeof(unsigned long long), s);
    if (rc) return rc;
    rc = runs_count(ev, a, found, s);
    if (!rc && *found && capacity) {
        rc = runs_store(ev, a, d_runs, capacity, s);
        if (!rc) FSEA_HIP(hipStreamSynchronize(s));
    }
    if (rc) return rc;
    ev->rows += a.n_rows;
    return ev->scratch.release(s);
}

int check_paint(const fsea_events *ev, const fsea_events_run *runs, const uint8_t *values, size_t n_runs, size_t n_rows,
                const uint8_t *image, size_t pitch) {
    if (!ev) return fail(FSEA_EINVAL, "events is NULL");
    if (int rc = fsea_detail::check_rows_head(nullptr, 0, n_rows)) return rc;
    if (n_runs > ((size_t)1 << 32)) return fail(FSEA_EINVAL, "n_runs %zu is more than 2^32", n_runs);
    if (n_runs && (!runs || !values)) return fail(FSEA_EINVAL, "NULL buffer for the %zu runs of the call", n_runs);
    if (n_rows == 0) return FSEA_OK;
    return fsea_detail::check_rows_planes(ev->width, n_rows, "image ", fsea_detail::RowPlane{image, "pitch", pitch});
}

// the zero fill and the runs, asynchronous on `s`
int paint_launch(const fsea_events *ev, const fsea_events_run *d_runs, const uint8_t *d_values, size_t n_runs, uint64_t row0,
                 size_t n_rows, uint8_t *d_image, size_t pitch, hipStream_t s) {
    const size_t width = (size_t)ev->width;
    if (pitch == width) FSEA_HIP(hipMemsetAsync(d_image, 0, n_rows * width, s));
    else FSEA_HIP(hipMemset2DAsync(d_image, pitch, 0, width, n_rows, s));
    if (n_runs == 0) return FSEA_OK;
    hipLaunchKernelGGL(fsea_events_paint, dim3((unsigned)((n_runs + EV_WAVES - 1) / EV_WAVES)), dim3(EV_WG), 0, s, d_runs, d_values,
                       n_runs, (unsigned long long)row0, n_rows, ev->width, d_image, pitch);
    FSEA_HIP(hipGetLastError());
    return FSEA_OK;
}

// union-find over run numbers, path halving; the lower number becomes the root, so a root is its event's first run
uint32_t find_root(std::vector<uint32_t> &parent, uint32_t i) {
    while (parent[i] != i) {
        parent[i] = parent[parent[i]];
        i = parent[i];
    }
    return i;
}

}  // namespace

extern "C" {

int fsea_events_create(fsea_events **out, int width, int device) {
    if (!out) return fail(FSEA_EINVAL, "events out-pointer is NULL");
    *out = nullptr;
    if (width < 1 || width > FSEA_EVENTS_MAX_WIDTH) {
        return fail(FSEA_EINVAL, "width must be in [1, %d], got %d", FSEA_EVENTS_MAX_WIDTH, width);
    }
    return fsea_detail::create_object(out, device, "fsea_events_create", [&](fsea_events *ev) -> int {
        ev->width = width;
        const hipError_t e = ev->scratch.create(ev->staging.stream);
        if (e != hipSuccess) return fsea_detail::init_code("fsea_events_create", e);
        if (int rc = ev->h_total.grow(sizeof(unsigned long long))) return rc;
        FSEA_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&ev->d_total), ev->h_total.ptr, 0));
        return ev->scratch.reserve(counts_bytes(EV_TILE) + sizeof(unsigned long long));
    });
}

int fsea_events_destroy(fsea_events *ev) { return fsea_detail::destroy_object(ev); }

int fsea_events_reset(fsea_events *ev) {
    return fsea_detail::reset_object(ev, "events is NULL", [&] {
        ev->rows = 0;
        return (int)FSEA_OK;
    });
}

int fsea_events_set_gap(fsea_events *ev, int gap_cols) {
    if (!ev) return fail(FSEA_EINVAL, "events is NULL");
    if (gap_cols < 0 || gap_cols > FSEA_EVENTS_MAX_GAP_COLS) {
        return fail(FSEA_EINVAL, "gap_cols must be in [0, %d], got %d", FSEA_EVENTS_MAX_GAP_COLS, gap_cols);
    }
    std::lock_guard<std::mutex> lock(ev->mu);
    ev->gap = gap_cols;
    return FSEA_OK;
}

int fsea_events_width(const fsea_events *ev) { return ev ? ev->width : 0; }

uint64_t fsea_events_rows(const fsea_events *ev) { return ev ? ev->rows : 0; }

int fsea_events_runs_device(fsea_events *ev, const uint8_t *d_mask, size_t mask_pitch, const void *d_levels, int type,
                            size_t level_pitch, size_t n_rows, fsea_events_run *d_runs, size_t capacity, size_t *n_runs, void *stream) {
    int rc = check_runs(ev, d_mask, mask_pitch, d_levels, type, level_pitch, n_rows, d_runs, capacity, n_runs);
    if (!rc && n_rows) rc = fsea_detail::check_aligned16("d_mask, d_levels and d_runs", d_mask, d_levels, d_runs);
    if (rc) return rc;
    *n_runs = 0;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(ev->mu);
    if ((rc = fsea_detail::check_rows_room(ev, n_rows))) return rc;
    FSEA_ON_DEVICE(ev->device);
    unsigned long long found = 0;
    rc = runs_launch(ev, RowsArgs{d_mask, mask_pitch, d_levels, type, level_pitch, n_rows}, d_runs, capacity, &found,
                     static_cast<hipStream_t>(stream));
    if (rc) return rc;
    *n_runs = (size_t)found;
    return FSEA_OK;
}

int fsea_events_runs_host(fsea_events *ev, const uint8_t *mask, size_t mask_pitch, const void *levels, int type, size_t level_pitch,
                          size_t n_rows, fsea_events_run *runs, size_t capacity, size_t *n_runs) {
    int rc = check_runs(ev, mask, mask_pitch, levels, type, level_pitch, n_rows, runs, capacity, n_runs);
    if (rc) return rc;
    *n_runs = 0;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(ev->mu);
    if ((rc = fsea_detail::check_rows_room(ev, n_rows))) return rc;
    FSEA_ON_DEVICE(ev->device);
    // mask and levels go up packed, the levels of a chunk behind its mask; the records of a chunk that still fit the
    // capacity come back behind it
    fsea_detail::HostStaging &st = ev->staging;
    const size_t width = (size_t)ev->width, esz = fsea_detail::row_elem_bytes(type);
    const fsea_detail::PackedPlane m(mask, mask_pitch, width), l(levels, level_pitch * esz, width * esz);
    const size_t mrow = m.packed, lrow = l.packed;
    size_t found = 0, written = 0;
    rc = fsea_detail::for_row_chunks(n_rows, mrow + lrow, [&](size_t r0, size_t nr) -> int {
        int rc = st.reserve(nr * (mrow + lrow), 0);
        if (rc) return rc;
        char *h = static_cast<char *>(st.h_in.ptr);
        m.pack(h, r0, nr);
        if (levels) l.pack(h + nr * mrow, r0, nr);
        FSEA_HIP(hipMemcpyAsync(st.d_in.ptr, h, nr * (mrow + lrow), hipMemcpyHostToDevice, st.stream));
        const char *d = static_cast<const char *>(st.d_in.ptr);
        const RowsArgs a{reinterpret_cast<const uint8_t *>(d), mrow, levels ? d + nr * mrow : nullptr, type, lrow / esz, nr};
        if ((rc = ev->scratch.acquire(counts_bytes(nr) + n_tiles_of(nr) * sizeof(unsigned long long), st.stream))) return rc;
        unsigned long long here = 0;
        if ((rc = runs_count(ev, a, &here, st.stream))) return rc;
        const size_t take = (size_t)std::min<unsigned long long>(here, capacity - written);
        if (take) {
            if ((rc = st.reserve(nr * (mrow + lrow), take * sizeof(fsea_events_run)))) return rc;
            if ((rc = runs_store(ev, a, static_cast<fsea_events_run *>(st.d_out.ptr), take, st.stream))) return rc;
            FSEA_HIP(hipMemcpyAsync(st.h_out.ptr, st.d_out.ptr, take * sizeof(fsea_events_run), hipMemcpyDeviceToHost, st.stream));
            FSEA_HIP(hipStreamSynchronize(st.stream));
            std::memcpy(runs + written, st.h_out.ptr, take * sizeof(fsea_events_run));
            written += take;
        }
        ev->rows += nr;
        found += (size_t)here;
        return ev->scratch.release(st.stream);
    });
    if (!rc) *n_runs = found;
    return rc;
}

int fsea_events_link(const fsea_events_run *runs, size_t n_runs, int gap_cols, int gap_rows, uint32_t min_rows, uint32_t min_cols,
                     uint64_t min_hits, uint32_t *event_of_run, fsea_events_event *events, size_t capacity, size_t *n_events) {
    if (!n_events || (!runs && n_runs) || (!events && capacity)) return fail(FSEA_EINVAL, "NULL buffer");
    if (n_runs >= 0xffffffffull) return fail(FSEA_EINVAL, "n_runs %zu is more than 2^32 - 2", n_runs);
    if (gap_cols < 0 || gap_cols > FSEA_EVENTS_MAX_GAP_COLS) {
        return fail(FSEA_EINVAL, "gap_cols must be in [0, %d], got %d", FSEA_EVENTS_MAX_GAP_COLS, gap_cols);
    }
    if (gap_rows < 0 || gap_rows > FSEA_EVENTS_MAX_GAP_ROWS) {
        return fail(FSEA_EINVAL, "gap_rows must be in [0, %d], got %d", FSEA_EVENTS_MAX_GAP_ROWS, gap_rows);
    }
    if (min_rows < 1) return fail(FSEA_EINVAL, "min_rows must be at least 1");
    if (min_cols < 1) return fail(FSEA_EINVAL, "min_cols must be at least 1");
    if (min_hits < 1) return fail(FSEA_EINVAL, "min_hits must be at least 1");
    for (size_t i = 0; i < n_runs; ++i) {
        if (runs[i].first > runs[i].last) return fail(FSEA_EINVAL, "run %zu: first %u is above last %u", i, runs[i].first, runs[i].last);
        if (i && (runs[i].row < runs[i - 1].row || (runs[i].row == runs[i - 1].row && runs[i].first <= runs[i - 1].last))) {
            return fail(FSEA_EINVAL, "runs are not sorted by (row, first) and disjoint: run %zu", i);
        }
    }
    *n_events = 0;
    const uint32_t n = (uint32_t)n_runs;
    const uint64_t G = (uint64_t)gap_cols;
    std::vector<uint32_t> parent, row_start, event_of_root;
    std::vector<fsea_events_event> all;
    try {
        parent.resize(n);
        // row_start[k]: the first run of the k-th distinct row, and n behind the last
        for (uint32_t i = 0; i < n; ++i) {
            parent[i] = i;
            if (i == 0 || runs[i].row != runs[i - 1].row) row_start.push_back(i);
        }
        row_start.push_back(n);
        // each row against the distinct rows at most gap_rows + 1 below it: both lists are sorted and disjoint, so the first
        // run of the lower row that can touch run a moves up with a, and the runs that touch a follow it
        const size_t n_distinct = row_start.size() - 1;
        for (size_t k = 0; k < n_distinct; ++k) {
            const uint64_t row = runs[row_start[k]].row;
            for (size_t m = k + 1; m < n_distinct && (uint64_t)runs[row_start[m]].row - row <= (uint64_t)gap_rows + 1; ++m) {
                uint32_t from = row_start[m];
                const uint32_t end = row_start[m + 1];
                for (uint32_t a = row_start[k]; a < row_start[k + 1] && from < end; ++a) {
                    while (from < end && (uint64_t)runs[from].last + G < runs[a].first) ++from;
                    for (uint32_t b = from; b < end && runs[b].first <= (uint64_t)runs[a].last + G; ++b) {
                        const uint32_t ra = find_root(parent, a), rb = find_root(parent, b);
                        if (ra < rb) parent[rb] = ra;
                        else parent[ra] = rb;
                    }
                }
            }
        }
        // the events in the order of their first runs; the runs come by in (row, first) order, so the first strict maximum is
        // the peak of the lowest row, then of the lowest column
        event_of_root.assign(n, 0xffffffffu);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t root = find_root(parent, i);
            const fsea_events_run &r = runs[i];
            if (root == i) {
                event_of_root[i] = (uint32_t)all.size();
                all.push_back(fsea_events_event{r.row, r.row, r.first, r.last, 1u, r.peak, r.row, r.peak_col, r.hits, r.level_sum});
                continue;
            }
            fsea_events_event &e = all[event_of_root[root]];
            e.row_last = std::max(e.row_last, r.row);
            e.col_first = std::min(e.col_first, r.first);
            e.col_last = std::max(e.col_last, r.last);
            e.runs += 1;
            e.hits += r.hits;
            e.level_sum = (int64_t)((uint64_t)e.level_sum + (uint64_t)r.level_sum);
            if (r.peak > e.peak) {
                e.peak = r.peak;
                e.peak_row = r.row;
                e.peak_col = r.peak_col;
            }
        }
    } catch (const std::bad_alloc &) {
        return fail(FSEA_ENOMEM, "out of host memory");
    }
    // the filters; the survivors are numbered in order
    size_t kept = 0;
    for (size_t j = 0; j < all.size(); ++j) {
        const fsea_events_event &e = all[j];
        const bool keep = (uint64_t)e.row_last - e.row_first + 1 >= min_rows && (uint64_t)e.col_last - e.col_first + 1 >= min_cols &&
                          e.hits >= min_hits;
        if (keep && kept < capacity) events[kept] = e;
        all[j].runs = keep ? (uint32_t)kept : 0xffffffffu;    // from here on: the event's number
        if (keep) ++kept;
    }
    if (event_of_run) {
        for (uint32_t i = 0; i < n; ++i) event_of_run[i] = all[event_of_root[find_root(parent, i)]].runs;
    }
    *n_events = kept;
    return FSEA_OK;
}

int fsea_events_paint_device(fsea_events *ev, const fsea_events_run *d_runs, const uint8_t *d_values, size_t n_runs, uint64_t row0,
                             size_t n_rows, uint8_t *d_image, size_t pitch, void *stream) {
    int rc = check_paint(ev, d_runs, d_values, n_runs, n_rows, d_image, pitch);
    if (!rc && n_rows) rc = fsea_detail::check_aligned16("d_runs and d_image", n_runs ? d_runs : nullptr, d_image);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(ev->mu);
    FSEA_ON_DEVICE(ev->device);
    return paint_launch(ev, d_runs, d_values, n_runs, row0, n_rows, d_image, pitch, static_cast<hipStream_t>(stream));
}

int fsea_events_paint_host(fsea_events *ev, const fsea_events_run *runs, const uint8_t *values, size_t n_runs, uint64_t row0,
                           size_t n_rows, uint8_t *image, size_t pitch) {
    int rc = check_paint(ev, runs, values, n_runs, n_rows, image, pitch);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(ev->mu);
    FSEA_ON_DEVICE(ev->device);
    // the image comes back tight, in chunks of rows; the runs and their values go up with each
    const size_t width = (size_t)ev->width, run_bytes = n_runs * sizeof(fsea_events_run);
    fsea_detail::HostStaging &st = ev->staging;
    return fsea_detail::for_row_chunks(n_rows, width, [&](size_t r0, size_t nr) -> int {
        int rc = st.reserve(run_bytes + n_runs, nr * width);
        if (rc) return rc;
        if (n_runs) {
            std::memcpy(st.h_in.ptr, runs, run_bytes);
            std::memcpy(static_cast<char *>(st.h_in.ptr) + run_bytes, values, n_runs);
            FSEA_HIP(hipMemcpyAsync(st.d_in.ptr, st.h_in.ptr, run_bytes + n_runs, hipMemcpyHostToDevice, st.stream));
        }
        const char *d = static_cast<const char *>(st.d_in.ptr);
        rc = paint_launch(ev, reinterpret_cast<const fsea_events_run *>(d), reinterpret_cast<const uint8_t *>(d) + run_bytes, n_runs,
                          row0 + r0, nr, static_cast<uint8_t *>(st.d_out.ptr), width, st.stream);
        if (rc) return rc;
        FSEA_HIP(hipMemcpyAsync(st.h_out.ptr, st.d_out.ptr, nr * width, hipMemcpyDeviceToHost, st.stream));
        FSEA_HIP(hipStreamSynchronize(st.stream));
        for (size_t r = 0; r < nr; ++r) std::memcpy(image + (r0 + r) * pitch, static_cast<const char *>(st.h_out.ptr) + r * width, width);
        return FSEA_OK;
    });
}

}  // extern "C"
