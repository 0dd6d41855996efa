// fsea_jobs.h -- what the objects that run a table of jobs over one resident buffer share: fsea_extract (fsea_extract.hip),
// fsea_measure (fsea_measure.hip) and fsea_audio (fsea_audio.hip).  The look-up of a workgroup's job on the device, the
// table's way from the caller to the device (JobTable: built in mapped host memory, copied by the one kernel
// fsea_jobs_upload, ordered by two events), the
// two numbers a table needs beside its entries, and the checks of a job table with the one text each has.  What a job is,
// what a kernel does with it and what lies behind the table in the scratch are each file's own.  Everything has internal
// linkage but jobs_upload, whose body stands beside its kernel in fsea_api.hip: the library is built without relocatable
// device code, so a kernel has one translation unit.
#pragma once

#include "fsea_internal.h"

namespace fsea_detail {

static_assert(FSEA_MEASURE_MAX_JOBS == FSEA_EXTRACT_MAX_JOBS && FSEA_AUDIO_MAX_JOBS == FSEA_EXTRACT_MAX_JOBS, "one cap of a job table");

// fsea_jobs_upload on `s`: n_words 32-bit words from mapped host memory (its host address) to device memory, one a lane
int jobs_upload(const void *h_table, void *d_table, uint32_t n_words, hipStream_t s);

namespace {

// The entry of a workgroup: the last of the n whose first tile is not behind `tile`; tile0[k] is entry k's first tile and
// steps = job_steps(n).  The answer lies in [lo, lo + len), len halves every step; the loads are uniform.
__device__ __forceinline__ int job_of_tile(const uint32_t *tile0, int n, int steps, uint32_t tile) {
    int lo = 0, len = n;
    for (int i = 0; i < steps; ++i) {
        const int half = len >> 1;
        if (half) {
            if (tile0[lo + half] <= tile) {
                lo += half;
                len -= half;
            } else {
                len = half;
            }
        }
    }
    return lo;
}

// ceil(log2(n)): the steps job_of_tile needs for n entries
int job_steps(size_t n) {
    int steps = 0;
    while (((size_t)1 << steps) < n) ++steps;
    return steps;
}

// the first tile of an entry of `count` elements in tiles of `tile`, *tiles the running total: <= 2^31 / tile + 65536 in all
uint32_t job_first_tile(uint64_t *tiles, uint64_t count, unsigned tile) {
    const uint32_t first = (uint32_t)*tiles;
    *tiles += (count + tile - 1) / tile;
    return first;
}

// The table of a call on its way to the device.  A call builds it in mapped host memory and fsea_jobs_upload copies it on the
// caller's stream in front of the object's kernels (3.6 us; a copy engine's transfer there cost two changes of queue, 6 to
// 10 us more a call: profiles/extract_rate.txt).  `copied` keeps the next call's fill behind this call's upload, the
// scratch's event every call behind the previous user of the device memory.  The caller holds the object's mutex.
struct JobTable {
    SharedScratch scratch;   // the device table and what an object keeps behind it
    MappedBuffer h_table;    // where a call builds the table
    Event copied;            // recorded behind fsea_jobs_upload

    hipError_t create(hipStream_t first) {
        hipError_t e = scratch.create(first);
        if (e == hipSuccess) e = copied.create();
        return e == hipSuccess ? hipEventRecord(copied, first) : e;
    }
    // a call begins: the previous call's upload has read the host table; table_bytes of it behind *host, to be filled
    template <class T>
    int begin(size_t table_bytes, T **host) {
        FSEA_HIP(hipEventSynchronize(copied));
        const int rc = h_table.grow(table_bytes);
        *host = static_cast<T *>(h_table.ptr);
        return rc;
    }
    // the filled table to the head of total_bytes >= table_bytes of scratch, on `s`; *base is the scratch
    int queue(size_t table_bytes, size_t total_bytes, hipStream_t s, uint8_t **base) {
        if (int rc = scratch.acquire(total_bytes, s)) return rc;
        if (int rc = jobs_upload(h_table.ptr, scratch.buf.ptr, (uint32_t)(table_bytes / sizeof(uint32_t)), s)) return rc;   // <= 65536 * 33 words
        FSEA_HIP(hipEventRecord(copied, s));
        *base = static_cast<uint8_t *>(scratch.buf.ptr);
        return FSEA_OK;
    }
    // behind the object's last launch of the call
    int release(hipStream_t s) { return scratch.release(s); }
};

// The checks of a job table, in the order both objects have them: the count
int check_jobs_count(size_t n_jobs) {
    if (n_jobs > FSEA_EXTRACT_MAX_JOBS) return fail(FSEA_EINVAL, "n_jobs %zu above %d", n_jobs, FSEA_EXTRACT_MAX_JOBS);
    return FSEA_OK;
}

// object (`name`: "extract", "measure" or "audio"), count, table and the two buffers of a run; no jobs: a no-op, nothing more is looked at
int check_jobs_head(const void *obj, const char *name, size_t n_jobs, const void *jobs, const void *in, const void *out) {
    if (!obj) return fail(FSEA_EINVAL, "%s is NULL", name);
    if (int rc = check_jobs_count(n_jobs)) return rc;
    if (n_jobs == 0) return FSEA_OK;
    if (!jobs) return fail(FSEA_EINVAL, "NULL job table");
    if (!in || !out) return fail(FSEA_EINVAL, "NULL buffer");
    return FSEA_OK;
}

// Job i's n elements from `first` inside the n_buffer of the call, wrap-safe, then n against its cap.  `elems`: "samples" or
// "pairs"; `buffer`: "input" or "buffer".
int check_job_span(size_t i, uint64_t first, uint64_t n, size_t n_buffer, uint64_t most, const char *elems, const char *buffer) {
    if (n > n_buffer || first > n_buffer - n) {
        return fail(FSEA_EINVAL, "job %zu: %s %llu .. %llu + %llu lie past the %zu of the %s", i, elems, (unsigned long long)first,
                    (unsigned long long)first, (unsigned long long)n, n_buffer, buffer);
    }
    if (n > most) return fail(FSEA_EINVAL, "job %zu: n_%s %llu too large", i, elems, (unsigned long long)n);
    return FSEA_OK;
}

// the elements of one call; `elems`: "outputs" or "pairs"
int check_jobs_total(uint64_t total, const char *elems) {
    if (total > (uint64_t)1 << 31) return fail(FSEA_EINVAL, "%llu %s in one call: more than 2^31", (unsigned long long)total, elems);
    return FSEA_OK;
}

}  // namespace

}  // namespace fsea_detail
