// fsea_rows.h -- what the objects that consume rows of levels share: fsea_persist (fsea_persist.hip), fsea_cfar
// (fsea_cfar.hip) and fsea_events (fsea_events.hip).  The common head of their structs, the limits of a call, the checks of
// the row arguments with the one text each has, the 16-byte-load predicate, the packing of host rows into the staging and
// the walk over its chunks, the zeroed accumulator of persist's counts and cfar's hits, and the two pieces of device code
// that the kernels have in common.  The group loaders of the three kernels are not here: their shapes differ for the
// reasons each file's head gives.  What only the two CFAR detectors share (fsea_cfar.hip and fsea_oscfar.hip: the object, its
// launch, the entry points, the kernels' geometry and signature) is in fsea_cfar_shared.h, on top of this header; the
// detector down the time axis (fsea_tcfar.hip) takes its part of both.
//
// Everything has internal linkage: the libraries export what they did before this header.
#pragma once

#include "fsea_internal.h"

#include <algorithm>
#include <cstddef>

namespace fsea_detail {

// How each of the three structs begins.  tests/test_persist_host.py, test_cfar_host.py and test_events_host.py reach the
// checks that read these with a fake object; an object's own settings follow at offset 16.
struct RowObject {
    int width = 0;
    int device = 0;
    uint64_t rows = 0;                            // rows offered since create or reset
};
static_assert(sizeof(RowObject) == 16 && offsetof(RowObject, device) == 4 && offsetof(RowObject, rows) == 8, "the fake objects of the tests");

constexpr size_t ROWS_MAX_CALL = (size_t)1 << 31;      // rows of one call
constexpr size_t ROWS_MAX_SPAN = (size_t)1 << 40;      // elements from the first row of a call to behind its last
constexpr size_t ROWS_STAGE_BYTES = (size_t)64 << 20;  // the host forms' chunk
constexpr int CFAR_LEVEL_LIMIT = 1 << 20;              // |level| of an f32 cell at most
static_assert(FSEA_PERSIST_U8 == FSEA_CFAR_U8 && FSEA_PERSIST_F32 == FSEA_CFAR_F32, "one pair of row types");
static_assert(FSEA_CFAR_F32_SCALE == 64 && FSEA_CFAR_MAX_OFFSET == CFAR_LEVEL_LIMIT, "the 32-bit bounds of the decision");

namespace {

size_t row_elem_bytes(int type) { return type == FSEA_CFAR_F32 ? 4 : 1; }

// One plane of rows as an entry point names it: `pitch_name` is "pitch", "mask pitch" or "level pitch".  A plane without a
// buffer (the optional levels) is not checked.
struct RowPlane {
    const void *buf;
    const char *pitch_name;
    size_t pitch;
};

// Type and count of the rows of a call.  `type_word`: "row" or "level"; null where the rows have no type (an image).
int check_rows_head(const char *type_word, int type, size_t n_rows) {
    if (type_word && type != FSEA_CFAR_U8 && type != FSEA_CFAR_F32) return fail(FSEA_EINVAL, "unknown %s type %d", type_word, type);
    if (n_rows > ROWS_MAX_CALL) return fail(FSEA_EINVAL, "n_rows %zu is more than 2^31", n_rows);
    return FSEA_OK;
}

// Buffer, pitches and span of the n_rows > 0 rows of a call, in that order.  `what`: "", "mask " or "image ", the rows the
// first plane holds.  A call with a second plane names no pitch in the span's text.
int check_rows_planes(int width, size_t n_rows, const char *what, const RowPlane &a, const RowPlane *b = nullptr) {
    if (!a.buf) return fail(FSEA_EINVAL, "NULL buffer for the %zu %srows of the call", n_rows, what);
    if (a.pitch < (size_t)width) return fail(FSEA_EINVAL, "%s %zu is below the width %d", a.pitch_name, a.pitch, width);
    if (b && b->buf && b->pitch < (size_t)width) return fail(FSEA_EINVAL, "%s %zu is below the width %d", b->pitch_name, b->pitch, width);
    const size_t most = ROWS_MAX_SPAN / n_rows;
    if (b ? a.pitch > most || (b->buf && b->pitch > most) : a.pitch > most) {
        return b ? fail(FSEA_EINVAL, "pitch x n_rows %zu is too large", n_rows)
                 : fail(FSEA_EINVAL, "pitch %zu x n_rows %zu is too large", a.pitch, n_rows);
    }
    return FSEA_OK;
}

// fsea_persist_add_* and fsea_cfar_add_*: the object (`name` for its text), then the rows
int check_rows_add(const RowObject *o, const char *name, const void *rows, int type, size_t n_rows, size_t pitch) {
    if (!o) return fail(FSEA_EINVAL, "%s is NULL", name);
    if (int rc = check_rows_head("row", type, n_rows)) return rc;
    return n_rows ? check_rows_planes(o->width, n_rows, "", RowPlane{rows, "pitch", pitch}) : (int)FSEA_OK;
}

// the caller holds the object's mutex
int check_rows_room(const RowObject *o, size_t n_rows) {
    if (o->rows + n_rows > 0xffffffffull) {
        return fail(FSEA_EINVAL, "n_rows %zu would take rows past 2^32 - 1 (%llu so far)", n_rows, (unsigned long long)o->rows);
    }
    return FSEA_OK;
}

// whether a launch may read the rows behind `base` with 16-byte loads
bool rows_vec16(const void *base, size_t pitch_bytes) { return ((uintptr_t)base & 15) == 0 && pitch_bytes % 16 == 0; }

// One plane of host rows on its way into the staging: `row_bytes` of every row, packed at a pitch of whole 16-byte groups
// (`packed`), the tail of a group zeroed.  No buffer: no bytes.
struct PackedPlane {
    const char *src;
    size_t pitch_bytes, row_bytes, packed;

    PackedPlane(const void *rows, size_t pitch_bytes_, size_t row_bytes_)
        : src(static_cast<const char *>(rows)), pitch_bytes(pitch_bytes_), row_bytes(row_bytes_),
          packed(rows ? (row_bytes_ + 15) & ~(size_t)15 : 0) {}
    // rows r0 .. r0 + nr - 1 to dst
    void pack(void *dst, size_t r0, size_t nr) const {
        char *d = static_cast<char *>(dst);
        for (size_t r = 0; r < nr; ++r) {
            std::memcpy(d + r * packed, src + (r0 + r) * pitch_bytes, row_bytes);
            std::memset(d + r * packed + row_bytes, 0, packed - row_bytes);
        }
    }
};

// body(r0, nr) -> FSEA_* code for the chunks of at most ROWS_STAGE_BYTES that n_rows rows of `bytes_per_row` make
template <class Body>
int for_row_chunks(size_t n_rows, size_t bytes_per_row, Body &&body) {
    const size_t chunk = std::max<size_t>(1, ROWS_STAGE_BYTES / bytes_per_row);
    for (size_t r0 = 0; r0 < n_rows; r0 += chunk) {
        if (int rc = body(r0, std::min(chunk, n_rows - r0))) return rc;
    }
    return FSEA_OK;
}

// A SharedScratch of a fixed size that starts zeroed and is added to by every launch: persist's counts, cfar's hits.  Its
// event orders the calls.
struct ZeroedScratch : SharedScratch {
    size_t bytes = 0;

    // in an object's initialiser (create_object), `what` the entry point's name; the zeroes are in place on return
    int create_zeroed(const char *what, size_t n_bytes, hipStream_t first) {
        bytes = n_bytes;
        hipError_t e = create(first);
        if (e != hipSuccess) return init_code(what, e);
        if (int rc = reserve(bytes)) return rc;
        e = hipMemset(buf.ptr, 0, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        return init_code(what, e);
    }
    // in an object's reset (reset_object), between its two waits for the device
    int zero() {
        FSEA_HIP(hipMemset(buf.ptr, 0, bytes));
        return FSEA_OK;
    }
    // the whole of it to `host` through the object's staging, behind every launch queued so far
    int fetch(HostStaging &staging, void *host) {
        const HostStaging::Part part[1] = {{host, bytes}};
        return staging.run(0, part, [](void *) {}, [&](void *, void **d_parts, hipStream_t s) {
            d_parts[0] = buf.ptr;                 // the object's own memory
            return acquire(s);
        });
    }
};

// fsea_cfar's level of an f32 element, which fsea_events sums under its runs: one rounded multiplication, round half to
// even; the clamp for a NaN
__device__ __forceinline__ int cfar_level_f32(float v) {
    const float t = __fmul_rn(v, (float)FSEA_CFAR_F32_SCALE);
    if (t != t || t <= (float)-CFAR_LEVEL_LIMIT) return -CFAR_LEVEL_LIMIT;
    if (t >= (float)CFAR_LEVEL_LIMIT) return CFAR_LEVEL_LIMIT;
    return (int)rintf(t);
}

// The rows of a workgroup's run where blockIdx.x counts runs of RUN rows: the first one to *row0, their number (fewer than
// RUN at the end of the call) returned
template <int RUN>
__device__ __forceinline__ int run_of_workgroup(size_t n_rows, size_t *row0) {
    *row0 = (size_t)blockIdx.x * RUN;
    const size_t left = n_rows - *row0;
    return left < (size_t)RUN ? (int)left : RUN;
}

}  // namespace

}  // namespace fsea_detail
