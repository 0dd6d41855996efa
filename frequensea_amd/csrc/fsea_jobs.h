// fsea_jobs.h -- what the objects that run a table of jobs over one resident buffer share: fsea_extract (fsea_extract.hip),
// fsea_measure (fsea_measure.hip), fsea_audio (fsea_audio.hip) and fsea_spectra (fsea_spectra.hip).  The look-up of a workgroup's job on the device; the
// table's way from the caller to the device (JobTable: records and first-tile column built in mapped host memory by the
// one routine `build`, copied by the one kernel fsea_jobs_upload, ordered by two events); the checks of a job table with
// the one text each has, the placement of the outputs among them; for the three objects that place their outputs
// (extract, audio, spectra), the layout and the host form that hands back only the jobs' own ranges; and, for the three that
// read pairs (measure, audio, spectra), the spans of laid-out extract jobs, the end of the staged input and the tail of
// run_device.  What a job is, what a kernel does with it, where its outputs lie and what lies behind the table in the
// scratch are each file's own.  Everything has internal linkage but
// jobs_upload, whose body stands beside its kernel in fsea_api.hip: the library is built without relocatable device code,
// so a kernel has one translation unit.
#pragma once

#include "fsea_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace fsea_detail {

static_assert(FSEA_MEASURE_MAX_JOBS == FSEA_EXTRACT_MAX_JOBS && FSEA_AUDIO_MAX_JOBS == FSEA_EXTRACT_MAX_JOBS &&
                  FSEA_SPECTRA_MAX_JOBS == FSEA_EXTRACT_MAX_JOBS,
              "one cap of a job table");

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
    // What a call's kernels get: the records, the column of their first tiles, the tiles of all, and the room behind the
    // table, which is there only for a call with behind_per_tile: otherwise `behind` may lie past the scratch
    template <class Rec>
    struct Built {
        const Rec *recs;
        const uint32_t *tile0;
        uint8_t *behind;
        uint64_t tiles;    // <= 2^31 / tile + 65536
    };
    // One call's table on `s`: n records, record r filled by fill(r, rec, first), which gets the entry's first tile and
    // returns its elements, in tiles of `tile`; fill is called exactly once for each r, in ascending order (extract's walks
    // its jobs alongside and skips those without output); the column of first tiles behind the records (an entry without
    // a tile has its successor's).  First the previous call's upload has read the host table; then the fill, the scratch, the upload.
    // behind_per_tile: bytes an object keeps behind the table for every tile, from a 64-byte boundary (measure's and spectra's partials).
    template <class Rec, class Fill>
    int build(size_t n, unsigned tile, size_t behind_per_tile, hipStream_t s, Fill &&fill, Built<Rec> *built) {
        const size_t bytes = n * (sizeof(Rec) + sizeof(uint32_t)), behind_at = (bytes + 63) & ~(size_t)63;   // <= 65536 * 33 words
        FSEA_HIP(hipEventSynchronize(copied));
        if (int rc = h_table.grow(bytes)) return rc;
        Rec *recs = static_cast<Rec *>(h_table.ptr);
        uint32_t *tile0 = reinterpret_cast<uint32_t *>(recs + n);
        uint64_t tiles = 0;
        for (size_t r = 0; r < n; ++r) {
            tile0[r] = (uint32_t)tiles;
            tiles += ((uint64_t)fill(r, recs[r], tile0[r]) + tile - 1) / tile;
        }
        if (int rc = scratch.acquire(behind_per_tile ? behind_at + (size_t)tiles * behind_per_tile : bytes, s)) return rc;
        if (int rc = jobs_upload(h_table.ptr, scratch.buf.ptr, (uint32_t)(bytes / sizeof(uint32_t)), s)) return rc;
        FSEA_HIP(hipEventRecord(copied, s));
        uint8_t *base = static_cast<uint8_t *>(scratch.buf.ptr);
        built->recs = reinterpret_cast<const Rec *>(base);
        built->tile0 = reinterpret_cast<const uint32_t *>(built->recs + n);
        built->behind = base + behind_at;
        built->tiles = tiles;
        return FSEA_OK;
    }
    // behind the object's last launch of the call
    int release(hipStream_t s) { return scratch.release(s); }
};

// The checks of a job table, in the order the four objects have them: the count
int check_jobs_count(size_t n_jobs) {
    if (n_jobs > FSEA_EXTRACT_MAX_JOBS) return fail(FSEA_EINVAL, "n_jobs %zu above %d", n_jobs, FSEA_EXTRACT_MAX_JOBS);
    return FSEA_OK;
}

// object (`name`: "extract", "measure", "audio" or "spectra"), count, table and the two buffers of a run; no jobs: a no-op, nothing more is looked at
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

// the offset of a pair stage
int check_offset(double offset_re, double offset_im) {
    if (!std::isfinite(offset_re) || !std::isfinite(offset_im)) return fail(FSEA_EINVAL, "the offset is not finite");
    return FSEA_OK;
}

// the elements of one call; `elems`: "outputs", "pairs" or "points"
int check_jobs_total(uint64_t total, const char *elems) {
    if (total > (uint64_t)1 << 31) return fail(FSEA_EINVAL, "%llu %s in one call: more than 2^31", (unsigned long long)total, elems);
    return FSEA_OK;
}

// Where the outputs of the jobs go, for the objects that place them: every job with an output inside the caller's
// `capacity`, in table order, then no two of them on top of one another.  at(i, &out_first, &n_out) says where job i's
// outputs lie; it may refuse the job for a reason of its own first (audio: the job's span), and that code is returned.  The
// text ends "lie past the <before><capacity><after>".
template <class At>
int check_jobs_placement(size_t n_jobs, size_t capacity, const char *before, const char *after, At &&at) {
    struct Placed {
        uint64_t first, n;
        uint32_t job;
    };
    std::vector<Placed> placed;
    for (size_t i = 0; i < n_jobs; ++i) {
        Placed p = {0, 0, (uint32_t)i};
        if (int rc = at(i, &p.first, &p.n)) return rc;
        if (p.n == 0) continue;
        if (p.n > capacity || p.first > capacity - p.n) {
            return fail(FSEA_EINVAL, "job %zu: outputs %llu .. %llu + %llu lie past the %s%zu%s", i, (unsigned long long)p.first,
                        (unsigned long long)p.first, (unsigned long long)p.n, before, capacity, after);
        }
        placed.push_back(p);
    }
    std::sort(placed.begin(), placed.end(), [](const Placed &a, const Placed &b) { return a.first != b.first ? a.first < b.first : a.job < b.job; });
    for (size_t k = 1; k < placed.size(); ++k) {
        const Placed &a = placed[k - 1], &b = placed[k];
        if (a.first + a.n > b.first) {
            return fail(FSEA_EINVAL, "the outputs of jobs %u and %u overlap", std::min(a.job, b.job), std::max(a.job, b.job));
        }
    }
    return FSEA_OK;
}

// fsea_X_layout: out_first of every job, back to back in table order, each at a multiple of `align` (a power of two);
// at(i, &out_first, &n_out) as above, of which only the count is taken: the out_first it reports is the one about to be
// overwritten, which a caller may have left unset, and is dropped.  `name` as in check_jobs_head, `total_name` the
// out-parameter's.
template <class Job, class At>
int layout_jobs(const void *obj, const char *name, Job *jobs, size_t n_jobs, size_t *total, const char *total_name, uint64_t align, At &&at) {
    if (!obj) return fail(FSEA_EINVAL, "%s is NULL", name);
    if (!total) return fail(FSEA_EINVAL, "%s is NULL", total_name);
    if (int rc = check_jobs_count(n_jobs)) return rc;
    if (n_jobs && !jobs) return fail(FSEA_EINVAL, "NULL job table");
    uint64_t end = 0, unused, n;
    for (size_t i = 0; i < n_jobs; ++i) {
        end = (end + align - 1) & ~(align - 1);
        at(i, &unused, &n);
        jobs[i].out_first = end;
        end += n;
    }
    *total = (size_t)end;
    return FSEA_OK;
}

// The host form of an object that places its outputs (`obj`: mu, device, staging), the arguments checked: in_bytes of
// input staged by fill(h_in), queue(d_in, d_out, stream), the elements in front of the end of the last placed job brought
// back, and of those only every job's own range to `out`; at(i, &out_first, &n_out) as above.  No output: nothing is done.
template <class T, class Out, class Fill, class Queue, class At>
int run_host_placed(T *obj, size_t in_bytes, size_t n_jobs, Out *out, Fill &&fill, Queue &&queue, At &&at) {
    uint64_t first = 0, n = 0;
    size_t end = 0;
    for (size_t i = 0; i < n_jobs; ++i) {
        at(i, &first, &n);
        if (n) end = std::max(end, (size_t)(first + n));
    }
    if (end == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(obj->mu);
    FSEA_ON_DEVICE(obj->device);
    const HostStaging::Part part[1] = {{out, end * sizeof(Out)}};
    return obj->staging.run(
        in_bytes, part, fill, [&](void *d_in, void **d_parts, hipStream_t s) { return queue(d_in, static_cast<Out *>(d_parts[0]), s); },
        [&](size_t, const uint8_t *h) {
            for (size_t i = 0; i < n_jobs; ++i) {
                at(i, &first, &n);
                if (n) std::memcpy(out + first, reinterpret_cast<const Out *>(h) + first, (size_t)n * sizeof(Out));
            }
        });
}

// fsea_X_jobs of a pair stage: the spans of the outputs of extract jobs that fsea_extract_layout laid out, each without its
// first skip_pairs pairs and of `most` pairs at the most; rest(job) fills what else the record has.
template <class Job, class Rest>
int jobs_of_extract(const fsea_extract_job *ejobs, size_t n_jobs, int decimation, size_t skip_pairs, unsigned most, Job *jobs, Rest &&rest) {
    if (int rc = check_jobs_count(n_jobs)) return rc;
    if (n_jobs && (!ejobs || !jobs)) return fail(FSEA_EINVAL, "NULL job table");
    if (decimation < 1) return fail(FSEA_EINVAL, "decimation must be at least 1, got %d", decimation);
    for (size_t i = 0; i < n_jobs; ++i) {
        const uint64_t outs = ejobs[i].n_samples / (uint64_t)decimation;
        const uint64_t skip = std::min<uint64_t>(skip_pairs, outs);
        if (outs - skip > most) return fail(FSEA_EINVAL, "job %zu: %llu pairs, more than %u", i, (unsigned long long)(outs - skip), most);
        jobs[i].first_pair = ejobs[i].out_first + skip;
        jobs[i].n_pairs = outs - skip;
        rest(jobs[i]);
    }
    return FSEA_OK;
}

// The host form of a pair stage stages the pairs in front of this: the end of the last job that has_output(job)
template <class Job, class Has>
size_t staged_pairs(const Job *jobs, size_t n_jobs, Has &&has_output) {
    size_t end = 0;
    for (size_t i = 0; i < n_jobs; ++i) {
        if (has_output(jobs[i])) end = std::max(end, (size_t)(jobs[i].first_pair + jobs[i].n_pairs));
    }
    return end;
}

// The tail of a pair stage's run_device, the arguments checked and n_jobs at least 1: the alignment of the two buffers
// (`out_name` has to be `align`-byte aligned), then queue(stream) under the object's mutex and on its device.
template <class T, class Queue>
int run_device_pairs(T *obj, const void *d_pairs, const void *d_out, const char *out_name, unsigned align, void *stream, Queue &&queue) {
    if (((uintptr_t)d_pairs & 7) || ((uintptr_t)d_out & (align - 1))) {
        return fail(FSEA_EINVAL, "d_pairs must be 8-byte and %s %u-byte aligned", out_name, align);
    }
    std::lock_guard<std::mutex> lock(obj->mu);
    FSEA_ON_DEVICE(obj->device);
    return queue(static_cast<hipStream_t>(stream));
}

}  // namespace

}  // namespace fsea_detail
