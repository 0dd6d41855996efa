// fsea_extract.hip -- event cut-outs (include/fsea.h: fsea_extract_*): a table of shift -> low-pass -> keep every D-th sample
// jobs over one resident 8-bit recording, every job with its own start, length, centre frequency and place in the output,
// all in one launch.  fsea_events_link says where the emissions are; this turns each box back into its signal.  No state
// between calls: a job's pairs are what a freshly reset fsea_zoom writes for the same samples, bit for bit.
//
// Kernel fsea_extract_u8 ("Event cut-outs"): one workgroup of ZM_WG = 256 lanes per tile of ZM_T = 128
// outputs of one job; the grid is the sum of the jobs' tiles.  The host turns every job that has an output into a 128-byte
// record (first, out_first, its first tile, its FirRot with the eight step phasors) and a column of first tiles; a
// workgroup finds its job by a bisection over that column (fsea_jobs.h: job_of_tile), `steps` = ceil(log2(records)) <= 16
// loads, all of them uniform: scalar loads and SGPRs, and so is the record itself.  The table's build and way to the device
// and the checks of a job table are fsea_measure's and fsea_audio's too, the placement of the outputs, the layout and the
// host form fsea_audio's (fsea_jobs.h).  From there on it is the zoom's tile (fsea_zoom_image.h): the tile's T D + L - 1
// rotated samples phase-major in LDS, one FMA chain per output with taps and byte offsets from scalar loads, 8-byte
// stores, the three static LDS sizes.  What differs is the staging: the groups of eight are aligned to the
// buffer (first + s a multiple of 8), so that a group inside the job is one 16-byte load whatever first mod 8 is; the two
// ends go sample by sample, and what lies in front of the job is the zero tail (fsea_fir_stage.h: stage_group_at).  No wave
// waits for another, no atomics, every loop has its bound on entry.
#include "fsea_jobs.h"
#include "fsea_zoom_image.h"

#include <cmath>
#include <cstddef>
#include <string>

using fsea_detail::DeviceGuard;
using fsea_detail::fail;
using namespace fsea_zoom_image;

namespace {

// a job on the device; jobs without output have none
struct ExtractRec {
    long long first;       // element of d_iq that is the job's sample 0
    long long out_first;   // element of d_pairs that is the job's output 0
    uint32_t tile0;        // the job's first tile: workgroups tile0 .. tile0 + ceil(n_out / ZM_T) - 1 are its own
    uint32_t pad[3];
    FirRot rot;            // n_in: the job's samples
};
static_assert(sizeof(ExtractRec) == 128, "records are read by scalar loads, a whole number of 64-byte lines each");

template <int CAP>
__device__ __forceinline__ void extract_body(const void *__restrict__ in, uint32_t flip, const ExtractRec *__restrict__ recs,
                                             const uint32_t *__restrict__ tile0, int n_rec, int steps,
                                             const float *__restrict__ taps, const uint32_t *__restrict__ offs, int L, int D,
                                             cf *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) cf lds[CAP];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;

    const ExtractRec *rec = recs + fsea_detail::job_of_tile(tile0, n_rec, steps, tile);
    // the record field by field: uniform, so scalar loads
    FirRot rot;   // delta, phase0 and offset: what rot_base reads
    rot.delta = rec->rot.delta;
    rot.phase0 = rec->rot.phase0;
    rot.offset = rec->rot.offset;
    const long long first = rec->first, n = rec->rot.n_in;

    const int pitch = zoom_pitch(D, L);
    const long long n_out = n / D;
    const long long i0 = (long long)(tile - rec->tile0) * ZM_T;    // first output of the tile
    const long long left = n_out - i0;                             // outputs from there on: at least 1
    const int n_tile = left < ZM_T ? (int)left : ZM_T;
    const int span = n_tile * D + L - 1;                           // x_ext entries the tile reads, from i0 D
    const long long s_first = i0 * D - (L - 1);                    // job sample of x_ext[i0 D] (negative: the zero tail)
    const long long e_al = (first + s_first) & ~7LL;               // the 8-element group of the buffer it lies in
    const int groups = (int)((first + s_first - e_al + span + 7) >> 3);
    const int o = (int)((rot.offset + e_al - first) & 7);          // stream position mod 8 of every group's sample 0
    cf turned[8];                                                  // the step phasors in a group's order, in registers
#pragma unroll
    for (int j = 0; j < 8; ++j) turned[j] = rec->rot.step[(o + j) & 7];

    // stage: x_ext[i0 D + m], m < span, rotated, phase-major.  Every entry a stored output reads lies inside the job or its
    // zero tail: (n_out - 1) D + L - 1 < n + L - 1.
    for (int g = tid; g < groups; g += ZM_WG) {
        const long long s = e_al + 8LL * g - first;
        cf v[8];
        stage_group_at<FIR_IN_U8>(in, first, s, n, flip, rot, turned, o, v);
        zoom_store_group(lds, v, (int)(s - s_first), span, D, pitch);
    }
    __syncthreads();

    // the first two waves: lane i's output
    if (tid < ZM_T) {
        const cf acc = zoom_chain(lds + tid, taps, offs, L);
        if (tid < n_tile) out[rec->out_first + i0 + tid] = acc;
    }
}

}  // namespace

#define FSEA_EXTRACT_KERNEL(name, cap)                                                                                    \
    extern "C" __global__ __launch_bounds__(ZM_WG) void name(                                                             \
        const void *__restrict__ in, uint32_t flip, const ExtractRec *__restrict__ recs, const uint32_t *__restrict__ tile0, \
        int n_rec, int steps, const float *__restrict__ taps, const uint32_t *__restrict__ offs, int L, int D,            \
        cf *__restrict__ out) {                                                                                           \
        extract_body<cap>(in, flip, recs, tile0, n_rec, steps, taps, offs, L, D, out);                                    \
    }
FSEA_EXTRACT_KERNEL(fsea_extract_u8_s, ZM_CAP_S)
FSEA_EXTRACT_KERNEL(fsea_extract_u8_m, ZM_CAP_M)
FSEA_EXTRACT_KERNEL(fsea_extract_u8, ZM_CAP_L)

struct fsea_extract {
    int n_taps = 0;       // the three plain numbers first: the checks of a run read `decimation` and nothing else
    int decimation = 1;
    int device = 0;
    fsea_detail::DeviceArray<float> d_taps;       // ZM_TAPS_ALLOC floats, zeros past n_taps
    fsea_detail::DeviceArray<uint32_t> d_offs;    // ZM_TAPS_ALLOC byte offsets of the taps' samples in the LDS image
    fsea_detail::JobTable table;                  // the records and their first-tile column
    std::mutex mu;
    fsea_detail::HostStaging staging;             // the host form
};
static_assert(offsetof(fsea_extract, n_taps) == 0 && offsetof(fsea_extract, decimation) == 4 && offsetof(fsea_extract, device) == 8,
              "the fake object of tests/test_extract_host.py");

namespace {

// where job i's pairs lie, (out_first, count): the placement check's, the layout's and the host form's
auto placed(const fsea_extract *x, const fsea_extract_job *jobs) {
    return [x, jobs](size_t i, uint64_t *first, uint64_t *n) {
        *first = jobs[i].out_first;
        *n = jobs[i].n_samples / (uint64_t)x->decimation;
    };
}

// Everything a run checks, in the header's order, reading nothing of the object but its decimation.
int check_run(const fsea_extract *x, const void *iq, size_t n_iq, const fsea_extract_job *jobs, size_t n_jobs, const void *pairs,
              size_t capacity) {
    if (int rc = fsea_detail::check_jobs_head(x, "extract", n_jobs, jobs, iq, pairs)) return rc;
    if (n_jobs == 0) return FSEA_OK;
    const uint64_t D = (uint64_t)x->decimation;
    uint64_t total = 0;
    for (size_t i = 0; i < n_jobs; ++i) {
        const fsea_extract_job &j = jobs[i];
        if (int rc = fsea_detail::check_job_span(i, j.first, j.n_samples, n_iq, ZM_MAX_SAMPLES, "samples", "input")) return rc;
        if (check_shift(j.cycles_per_sample, j.phase0_cycles, j.sample_offset, (size_t)j.n_samples)) {
            const std::string why = fsea_last_error_string();
            return fail(FSEA_EINVAL, "job %zu: %s", i, why.c_str());
        }
        total += j.n_samples / D;
    }
    if (int rc = fsea_detail::check_jobs_total(total, "outputs")) return rc;
    return fsea_detail::check_jobs_placement(n_jobs, capacity, "capacity of ", " pairs", [&](size_t i, uint64_t *first, uint64_t *n) {
        placed(x, jobs)(i, first, n);
        return FSEA_OK;
    });
}

// One call on device buffers, asynchronous on `s`: the records built in mapped host memory, their upload, the launch.  The
// caller holds x->mu and is on x's device; the arguments are checked.
int queue_call(fsea_extract *x, const void *d_iq, int flip, const fsea_extract_job *jobs, size_t n_jobs, void *d_pairs, hipStream_t s) {
    const int D = x->decimation, L = x->n_taps;
    size_t n_rec = 0;
    for (size_t i = 0; i < n_jobs; ++i) n_rec += jobs[i].n_samples / (uint64_t)D ? 1 : 0;
    if (n_rec == 0) return FSEA_OK;
    size_t i = 0;   // the job of the next record: jobs without output have none
    fsea_detail::JobTable::Built<ExtractRec> t;
    const int rc = x->table.build<ExtractRec>(n_rec, ZM_T, 0, s, [&](size_t, ExtractRec &rec, uint32_t tile0) {
        while (jobs[i].n_samples / (uint64_t)D == 0) ++i;
        const fsea_extract_job &j = jobs[i++];
        rec.first = (long long)j.first;
        rec.out_first = (long long)j.out_first;
        rec.tile0 = tile0;
        rec.pad[0] = rec.pad[1] = rec.pad[2] = 0;
        rec.rot = make_rot(j.cycles_per_sample, j.phase0_cycles, j.sample_offset, (size_t)j.n_samples);
        return j.n_samples / (uint64_t)D;
    }, &t);
    if (rc) return rc;
    const int need = zoom_lds_samples(D, L);
    auto kernel = need <= ZM_CAP_S ? fsea_extract_u8_s : need <= ZM_CAP_M ? fsea_extract_u8_m : fsea_extract_u8;
    hipLaunchKernelGGL(kernel, dim3((unsigned)t.tiles), dim3(ZM_WG), 0, s, d_iq, flip ? 0x80808080u : 0u, t.recs, t.tile0, (int)n_rec,
                       fsea_detail::job_steps(n_rec), (const float *)x->d_taps.ptr, (const uint32_t *)x->d_offs.ptr, L, D,
                       static_cast<cf *>(d_pairs));
    FSEA_HIP(hipGetLastError());
    return x->table.release(s);
}

}  // namespace

extern "C" {

int fsea_extract_create(fsea_extract **out, const double *taps, int n_taps, int decimation, int device) {
    if (!out) return fail(FSEA_EINVAL, "extract out-pointer is NULL");
    *out = nullptr;
    if (int rc = FirState::check_taps(taps, n_taps)) return rc;
    if (decimation < 1 || decimation > FSEA_ZOOM_MAX_DECIMATION) {
        return fail(FSEA_EINVAL, "decimation must be in [1, %d], got %d", FSEA_ZOOM_MAX_DECIMATION, decimation);
    }
    return fsea_detail::create_object(out, device, "fsea_extract_create", [&](fsea_extract *x) -> hipError_t {
        x->n_taps = n_taps;
        x->decimation = decimation;
        float tf[ZM_TAPS_ALLOC] = {};
        for (int k = 0; k < n_taps; ++k) tf[k] = (float)taps[k];
        uint32_t offs[ZM_TAPS_ALLOC];
        zoom_fill_offsets(offs, n_taps, decimation);
        hipError_t e = x->d_taps.upload(tf, ZM_TAPS_ALLOC);
        if (e == hipSuccess) e = x->d_offs.upload(offs, ZM_TAPS_ALLOC);
        if (e == hipSuccess) e = x->table.create(x->staging.stream);
        return e;
    });
}

int fsea_extract_destroy(fsea_extract *x) { return fsea_detail::destroy_object(x); }

int fsea_extract_decimation(const fsea_extract *x) { return x ? x->decimation : 0; }

int fsea_extract_n_taps(const fsea_extract *x) { return x ? x->n_taps : 0; }

size_t fsea_extract_out_pairs(const fsea_extract *x, size_t n_samples) { return x ? n_samples / (size_t)x->decimation : 0; }

size_t fsea_extract_lead(int n_taps, int decimation) {
    if (n_taps < 1 || decimation < 1) return 0;
    const size_t D = (size_t)decimation;
    return ((size_t)n_taps - 1 + D - 1) / D * D;
}

int fsea_extract_layout(const fsea_extract *x, fsea_extract_job *jobs, size_t n_jobs, size_t *total_pairs) {
    return fsea_detail::layout_jobs(x, "extract", jobs, n_jobs, total_pairs, "total_pairs", 2, placed(x, jobs));
}

int fsea_extract_run_device(fsea_extract *x, const void *d_iq, size_t n_iq_samples, int flip, const fsea_extract_job *jobs,
                            size_t n_jobs, void *d_pairs, size_t pairs_capacity, void *stream) {
    int rc = check_run(x, d_iq, n_iq_samples, jobs, n_jobs, d_pairs, pairs_capacity);
    if (!rc && n_jobs) rc = fsea_detail::check_aligned16("d_iq and d_pairs", d_iq, d_pairs);
    if (rc || n_jobs == 0) return rc;
    std::lock_guard<std::mutex> lock(x->mu);
    FSEA_ON_DEVICE(x->device);
    return queue_call(x, d_iq, flip, jobs, n_jobs, d_pairs, static_cast<hipStream_t>(stream));
}

int fsea_extract_run_host(fsea_extract *x, const uint8_t *iq, size_t n_iq_samples, int flip, const fsea_extract_job *jobs,
                          size_t n_jobs, float *pairs, size_t pairs_capacity) {
    const int rc = check_run(x, iq, n_iq_samples, jobs, n_jobs, pairs, pairs_capacity);
    if (rc || n_jobs == 0) return rc;
    return fsea_detail::run_host_placed(
        x, 2 * n_iq_samples, n_jobs, reinterpret_cast<cf *>(pairs), [&](void *h_in) { std::memcpy(h_in, iq, 2 * n_iq_samples); },
        [&](void *d_in, cf *d_out, hipStream_t s) { return queue_call(x, d_in, flip, jobs, n_jobs, d_out, s); },
        placed(x, jobs));
}

int fsea_extract_jobs(const fsea_events_event *events, size_t n_events, int width, int hop, uint64_t n_samples, int n_taps,
                      int decimation, double max_fill, fsea_extract_job *jobs, uint8_t *fits) {
    if (n_events && (!events || !jobs || !fits)) return fail(FSEA_EINVAL, "NULL events, jobs or fits");
    if (width < 1) return fail(FSEA_EINVAL, "width must be at least 1, got %d", width);
    if (hop < 1) return fail(FSEA_EINVAL, "hop must be at least 1, got %d", hop);
    if (n_taps < 1 || n_taps > FSEA_FIR_MAX_TAPS) return fail(FSEA_EINVAL, "n_taps must be in [1, %d], got %d", FSEA_FIR_MAX_TAPS, n_taps);
    if (decimation < 1 || decimation > FSEA_ZOOM_MAX_DECIMATION) {
        return fail(FSEA_EINVAL, "decimation must be in [1, %d], got %d", FSEA_ZOOM_MAX_DECIMATION, decimation);
    }
    if (!(max_fill > 0.0 && max_fill <= 1.0)) return fail(FSEA_EINVAL, "max_fill must be in (0, 1]");
    const uint64_t lead = fsea_extract_lead(n_taps, decimation), N = (uint64_t)width, H = (uint64_t)hop;
    for (size_t i = 0; i < n_events; ++i) {
        const fsea_events_event &e = events[i];
        fsea_extract_job &j = jobs[i];
        const uint64_t begin = (uint64_t)e.row_first * H;
        const uint64_t first = begin - std::min(begin, lead);
        const uint64_t end = std::min(n_samples, (uint64_t)e.row_last * H + N);
        const int64_t cols = (int64_t)e.col_last - (int64_t)e.col_first + 1;
        const int64_t off = (int64_t)e.col_first + (int64_t)e.col_last - 2 * (int64_t)(N / 2);   // twice the columns from the centre
        fits[i] = (double)(cols * decimation) <= max_fill * (double)N ? 1 : 0;
        j.first = j.sample_offset = first;
        j.n_samples = fits[i] && end > first ? end - first : 0;
        j.cycles_per_sample = (double)-off / (double)(2 * N);
        j.phase0_cycles = 0.0;
        j.out_first = 0;
    }
    return FSEA_OK;
}

}  // extern "C"
