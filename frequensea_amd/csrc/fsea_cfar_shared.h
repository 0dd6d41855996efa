// fsea_cfar_shared.h -- what the two CFAR detectors across frequency share: fsea_cfar (fsea_cfar.hip, cell averaging on
// prefix sums) and fsea_oscfar (fsea_oscfar.hip, a rank of the training cells).  A third user, fsea_tcfar (fsea_tcfar.hip,
// cell averaging down the time axis), takes level_at, spread4 and the entry points that need nothing but the object's head
// -- create, reset, the checks of set, hits_host -- and has a geometry, a kernel signature, an object and adds of its own
// (context rows, a fifth setting).  Included by those three files only.  On the device: the
// geometry of a workgroup, the level of a cell, the spreading of mask bits into bytes, the wave-local fence and the
// kernels' one signature.  On the host: the object, its one launch and the entry points that differ in nothing but the
// object's name and the kernels.  What is not here differs for the reasons each file's head gives: the group loaders, the
// staging (a prefix scan against plain levels), the decision, the fourth setting and the kernels' occupancy.
//
// The bookkeeping of a step's ballot, the mask stores and the end-of-run fold are the same text in both kernel bodies and
// are not here either: as member or free __forceinline__ functions they cost fsea_cfar's four kernels 4 to 10 vector
// registers each (profiles/cfar_shared_scaffold.txt), and what is here leaves all eight kernels instruction for instruction
// as they were.
//
// Everything has internal linkage, as in fsea_rows.h.
#pragma once

#include "fsea_rows.h"

namespace fsea_detail {

namespace {

// A workgroup of 256 lanes owns a tile of 1024 columns and a run of 64 rows; each of its four waves takes every fourth row.
constexpr int DET_WG = 256;                       // lanes per workgroup
constexpr int DET_WAVES = DET_WG / 64;
constexpr int DET_C = FSEA_CFAR_TILE_COLUMNS;     // columns per tile
constexpr int DET_RUN = FSEA_CFAR_RUN_ROWS;       // rows per workgroup
static_assert(FSEA_OSCFAR_TILE_COLUMNS == FSEA_CFAR_TILE_COLUMNS && FSEA_OSCFAR_RUN_ROWS == FSEA_CFAR_RUN_ROWS, "one geometry");
static_assert(DET_C == 16 * 64, "a wave decides a row of the tile in 16 steps; a lane stores 16 mask bytes");
static_assert(DET_RUN % DET_WAVES == 0 && DET_RUN / DET_WAVES <= 255, "a run is whole iterations of the four waves; a lane counts a column in a byte");

template <bool F32>
__device__ __forceinline__ int level_at(const void *__restrict__ rows, size_t i) {
    if (F32) return cfar_level_f32(static_cast<const float *>(rows)[i]);
    return (int)static_cast<const uint8_t *>(rows)[i];
}

// bits 0..3 of n to the bytes of a word, 255 for a set bit: the four shifted copies of n do not overlap
__device__ __forceinline__ uint32_t spread4(uint32_t n) { return (((n & 15u) * 0x00204081u) & 0x01010101u) * 255u; }

// The waves of a workgroup do not wait for one another: the staged arrays are a wave's own, an LDS instruction of a wave is
// carried out after the ones it issued before, and wave_sync() keeps the compiler from moving an access across it.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The one signature of the eight kernels; `fourth` is the method or the rank.
using DetectorKernel = void (*)(const void *, size_t, size_t, int, int, int, int, int, uint8_t *, int, uint32_t *, uint32_t *);

// A kernel `name` around the file's `body<F32, VEC>` and its `Settings`, BLOCKS workgroups to a SIMD's registers
#define FSEA_DETECTOR_KERNEL(name, body, BLOCKS, F32, VEC)                                                                     \
    extern "C" __global__ __launch_bounds__(fsea_detail::DET_WG, BLOCKS) void name(                                            \
        const void *__restrict__ rows, size_t n_rows, size_t pitch, int width, int guard, int train, int offset, int fourth,   \
        uint8_t *__restrict__ mask, int mask_vec, uint32_t *__restrict__ row_hits, uint32_t *__restrict__ hits) {              \
        body<F32, VEC>(rows, n_rows, pitch, width, Settings{guard, train, offset, fourth}, mask, mask_vec, row_hits, hits);    \
    }

// The object: `Settings` is four ints (guard, train, offset and the file's own fourth) with their defaults, at offset 16
// for the fake objects of the tests; the kernels are the 16-byte and the cell-by-cell one of each row type.
template <class Settings, DetectorKernel U8, DetectorKernel F32, DetectorKernel U8_NARROW, DetectorKernel F32_NARROW>
struct Detector : RowObject {
    Settings set;
    ZeroedScratch hits;                           // width u32; its event orders the calls
    std::mutex mu;
    HostStaging staging;                          // the host forms

    // One add on device rows, asynchronous on `s`.  The caller holds mu, is on the device and has checked the arguments.
    int add_launch(const void *d_rows, int type, size_t n_rows, size_t pitch, uint8_t *d_mask, uint32_t *d_row_hits, hipStream_t s) {
        int rc = hits.acquire(s);
        if (rc) return rc;
        if (d_row_hits) FSEA_HIP(hipMemsetAsync(d_row_hits, 0, n_rows * sizeof(uint32_t), s));   // set, not added to
        const dim3 grid((unsigned)((n_rows + DET_RUN - 1) / DET_RUN), (unsigned)((width + DET_C - 1) / DET_C));
        const bool vec = rows_vec16(d_rows, pitch * row_elem_bytes(type));
        const int mask_vec = width % 16 == 0;
        const auto [guard, train, offset, fourth] = set;
        const DetectorKernel kernel = type == FSEA_CFAR_U8 ? (vec ? U8 : U8_NARROW) : (vec ? F32 : F32_NARROW);
        hipLaunchKernelGGL(kernel, grid, dim3(DET_WG), 0, s, d_rows, n_rows, pitch, width, guard, train, offset, fourth, d_mask,
                           mask_vec, d_row_hits, static_cast<uint32_t *>(hits.buf.ptr));
        FSEA_HIP(hipGetLastError());
        rows += n_rows;
        return hits.release(s);
    }
};

// The entry points of a detector D (a Detector), `name` the object's word in the texts: "cfar" or "oscfar".

// `entry`: the entry point's name, for a failure's text
template <class D>
int detector_create(D **out, int width, int device, const char *name, const char *entry) {
    if (!out) return fail(FSEA_EINVAL, "%s out-pointer is NULL", name);
    *out = nullptr;
    if (width < 1 || width > FSEA_CFAR_MAX_WIDTH) {
        return fail(FSEA_EINVAL, "width must be in [1, %d], got %d", FSEA_CFAR_MAX_WIDTH, width);
    }
    return create_object(out, device, entry, [&](D *c) -> int {
        c->width = width;
        return c->hits.create_zeroed(entry, (size_t)width * sizeof(uint32_t), c->staging.stream);
    });
}

template <class D>
int detector_reset(D *c, const char *null_message) {
    return reset_object(c, null_message, [&] {
        c->rows = 0;
        return c->hits.zero();
    });
}

// fsea_X_set: the object and the three settings the detectors share, in that order; the fourth is the caller's
template <class D>
int detector_check_set(const D *c, const char *name, int guard, int train, int offset) {
    if (!c) return fail(FSEA_EINVAL, "%s is NULL", name);
    if (guard < 0 || guard > FSEA_CFAR_MAX_GUARD) return fail(FSEA_EINVAL, "guard must be in [0, %d], got %d", FSEA_CFAR_MAX_GUARD, guard);
    if (train < 1 || train > FSEA_CFAR_MAX_TRAIN) return fail(FSEA_EINVAL, "train must be in [1, %d], got %d", FSEA_CFAR_MAX_TRAIN, train);
    if (offset < -FSEA_CFAR_MAX_OFFSET || offset > FSEA_CFAR_MAX_OFFSET) {
        return fail(FSEA_EINVAL, "offset must be in [-%d, %d], got %d", FSEA_CFAR_MAX_OFFSET, FSEA_CFAR_MAX_OFFSET, offset);
    }
    return FSEA_OK;
}

template <class D>
int detector_add_device(D *c, const char *name, const void *d_rows, int type, size_t n_rows, size_t pitch, uint8_t *d_mask,
                        uint32_t *d_row_hits, void *stream) {
    int rc = check_rows_add(c, name, d_rows, type, n_rows, pitch);
    if (!rc && n_rows) rc = check_aligned16("d_rows, d_mask and d_row_hits", d_rows, d_mask, d_row_hits);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(c->mu);
    if ((rc = check_rows_room(c, n_rows))) return rc;
    FSEA_ON_DEVICE(c->device);
    return c->add_launch(d_rows, type, n_rows, pitch, d_mask, d_row_hits, static_cast<hipStream_t>(stream));
}

template <class D>
int detector_add_host(D *c, const char *name, const void *rows, int type, size_t n_rows, size_t pitch, uint8_t *mask,
                      uint32_t *row_hits) {
    int rc = check_rows_add(c, name, rows, type, n_rows, pitch);
    if (rc) return rc;
    if (n_rows == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(c->mu);
    if ((rc = check_rows_room(c, n_rows))) return rc;
    FSEA_ON_DEVICE(c->device);
    // the rows go up packed, in chunks; mask and row hits of a chunk come back behind it
    const size_t width = (size_t)c->width, esz = row_elem_bytes(type);
    const PackedPlane in(rows, pitch * esz, width * esz);
    return for_row_chunks(n_rows, in.packed, [&](size_t r0, size_t nr) {
        const HostStaging::Part parts[2] = {{mask ? mask + r0 * width : nullptr, nr * width},
                                            {row_hits ? row_hits + r0 : nullptr, nr * sizeof(uint32_t)}};
        return c->staging.run(
            nr * in.packed, parts, [&](void *h_in) { in.pack(h_in, r0, nr); },
            [&](void *d_in, void **d_parts, hipStream_t s) {
                return c->add_launch(d_in, type, nr, in.packed / esz, static_cast<uint8_t *>(d_parts[0]),
                                     static_cast<uint32_t *>(d_parts[1]), s);
            });
    });
}

template <class D>
int detector_hits_host(D *c, const char *name, uint32_t *hits) {
    if (!c) return fail(FSEA_EINVAL, "%s is NULL", name);
    if (!hits) return fail(FSEA_EINVAL, "hits is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    FSEA_ON_DEVICE(c->device);
    return c->hits.fetch(c->staging, hits);
}

}  // namespace

}  // namespace fsea_detail
