// fsea_audio.hip -- cut-out audio (include/fsea.h: fsea_audio_*): a table of jobs over one resident buffer of f32 pairs, one
// run of demodulated, low-passed and decimated audio per job -- the FM discriminator of the reference's WBFM chain or the AM
// envelope, then an L-tap real f64 filter that keeps every D-th value -- all jobs in one launch.  fsea_extract turns each box
// into its signal, fsea_measure says what is inside, this says what it carries.  No state between calls.  Every term is f64
// with the roundings the header writes out, so a job's audio is a function of its pairs alone, bit for bit.
//
// Kernel fsea_audio_tiles ("Cut-out audio"): one workgroup of AU_WG = 256 lanes per tile of T outputs of
// one job; the grid is the sum of the jobs' tiles.  T is the object's: the largest count up to 256 whose T D + L - 1
// discriminator values fit 4096 (audio_tile), as fsea_demod's stage 1 picks its own.  The device table is the caller's jobs
// as they are and a column of first tiles, built and brought there as the others' (fsea_jobs.h: JobTable); a workgroup
// finds its job by job_of_tile, scalar loads; the placement check, the layout and the host form are fsea_extract's too.
// Staging: the lanes stride over the tile's span of d_ext; each loads its pair and the pair before it (the neighbour
// lane's line: a cache hit), converts, subtracts and computes d once; what lies in front of the job is +0.0; an address
// in front of the job is the job's pair 0 and a select drops what it gave.  The values
// stand phase-major in LDS, value m of the span at [m mod D][m / D] with an odd pitch (the zoom's image, in doubles), so the
// 64 ds_read_b64 of a wave's tap k touch 64 consecutive doubles: no bank conflict at any D.  The staging's writes go down a
// column, rows `pitch` doubles apart: odd, so 16 lanes meet 16 different double-wide banks for D >= 16 and a 16 / D-way
// conflict below that, on a sixteenth of the LDS traffic.  One __syncthreads, then lane j < T runs output j's chain: taps
// and byte offsets from scalar loads of two device tables, one multiply and one add per tap, a 4-byte store.  No atomics, no
// wave waits for another but at that barrier, every loop has its bound on entry.
#include "fsea_fir_stage.h"
#include "fsea_jobs.h"

#include <algorithm>
#include <cmath>
#include <cstddef>

// every product and sum below is rounded on its own: a'a + b'b, c[k] d + acc and the like must not become one FMA
#pragma clang fp contract(off)

using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int AU_WG = 256;
constexpr int AU_SPAN = 4096;                               // discriminator values a tile may read
constexpr int AU_CAP = AU_SPAN + 2 * FSEA_AUDIO_MAX_DECIMATION;   // doubles of the LDS image: the last column and the odd pitch
static_assert(4 * AU_CAP * sizeof(double) <= 160 * 1024, "four workgroups per CU");
static_assert(sizeof(fsea_audio_job) == 24, "the record of include/fsea.h");

// outputs per workgroup: a tile's T D + L - 1 values fit AU_SPAN; at least 56 (D = 64, L = 512)
constexpr int audio_tile(int D, int L) { return std::min(AU_WG, (AU_SPAN - (L - 1)) / D); }
// columns of the phase-major image: value m of the tile at [m % D][m / D], m < T D + L - 1; odd
constexpr int audio_pitch(int D, int L) { return (audio_tile(D, L) + (L - 1 + D - 1) / D) | 1; }
static_assert(audio_tile(FSEA_AUDIO_MAX_DECIMATION, FSEA_FIR_MAX_TAPS) == 56 && audio_tile(1, 1) == AU_WG, "the tile sizes DESIGN.md names");
// D pitch <= D (T + (L - 1 + D - 1) / D + 1) <= T D + L - 1 + (D - 1) + D < AU_SPAN + 2 D
static_assert(FSEA_AUDIO_MAX_DECIMATION * audio_pitch(FSEA_AUDIO_MAX_DECIMATION, FSEA_FIR_MAX_TAPS) <= AU_CAP &&
              audio_pitch(1, FSEA_FIR_MAX_TAPS) <= AU_CAP, "the image fits at the corners");

constexpr double AU_C0 = 0.98419158358617365, AU_C1 = 0.093485702629671305, AU_C2 = 0.19556307900617517;
constexpr double AU_HALF_PI = 3.14159265358979323846 / 2;

// The discriminator's value for the pair (a, b) behind the pair (pa, pb): the reference's arctangent expression
// (src/nrf.c:971-991) without its ampl_conv factor; +0.0 where both products are zero (a silent pair).
__device__ __forceinline__ double discriminate(double pa, double pb, double a, double b) {
    const double real = pa * a + pb * b;
    double imag = pa * b - a * pb;
    bool minus = imag < 0.0;
    imag = minus ? -imag : imag;
    const bool silent = real == 0.0 && imag == 0.0;
    const bool eq = real == imag, gt = real > imag;      // neither holds with a NaN: the third branch, as in the reference
    const double num = gt ? imag : real, den = gt ? real : imag;
    const double div = eq ? 1.0 : __ddiv_rn(num, den);
    const double ang = eq || gt ? 0.0 : -AU_HALF_PI;
    minus = eq || gt ? minus : !minus;
    const double v = ang + __ddiv_rn(div, AU_C0 + div * (AU_C1 + div * AU_C2));
    return silent ? 0.0 : minus ? -v : v;
}

}  // namespace

// grid: the tiles of all jobs; tile0[k] is job k's first tile, a job's tiles follow one another.  T, pitch: audio_tile and
// audio_pitch of (D, L); offs[k]: the byte offset of tap k's value in the image from a lane's column.
extern "C" __global__ __launch_bounds__(AU_WG, 4) void fsea_audio_tiles(const float2 *__restrict__ pairs,
                                                                    const fsea_audio_job *__restrict__ jobs,
                                                                    const uint32_t *__restrict__ tile0, int n_jobs, int steps,
                                                                    int kind, const double *__restrict__ taps,
                                                                    const uint32_t *__restrict__ offs, int L, int D, int T,
                                                                    int pitch, double off_re, double off_im, double gain,
                                                                    float *__restrict__ audio) {
    __shared__ __attribute__((aligned(16))) double lds[AU_CAP];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;

    const int lo = fsea_detail::job_of_tile(tile0, n_jobs, steps, tile);
    const unsigned long long first = jobs[lo].first_pair, out_first = jobs[lo].out_first;
    const int n_out = (int)((unsigned)jobs[lo].n_pairs / (unsigned)D);   // at least 1: the job has a tile; n_pairs <= 2^24
    const int i0 = (int)(tile - tile0[lo]) * T;                 // first output of the tile
    const int left = n_out - i0;                                // outputs from there on: at least 1
    const int n_tile = left < T ? left : T;
    const int span = n_tile * D + L - 1;                        // d_ext entries the tile reads, from i0 D
    const int s_first = i0 * D - (L - 1);                       // the job's pair behind d_ext[i0 D] (negative: the zero prefix)
    const float2 *__restrict__ job = pairs + first;

    // stage: d_ext[i0 D + m], m < span, phase-major.  Every pair read lies inside the job: s <= n_out D - 1 < n_pairs.
    const int dq = AU_WG / D, dr = AU_WG - dq * D;
    int q = tid / D, r = tid - q * D;
    for (int m = tid; m < span; m += AU_WG) {
        const int s = s_first + m;
        const int at = s > 0 ? s : 0, before = s > 1 ? s - 1 : 0;
        const float2 z = job[at], w = job[before];
        const double a = (double)z.x - off_re, b = (double)z.y - off_im;
        double d;
        if (kind == FSEA_AUDIO_FM) {
            const double pa = (double)w.x - off_re, pb = (double)w.y - off_im;
            d = s > 0 ? discriminate(pa, pb, a, b) : 0.0;
        } else {
            d = s >= 0 ? __dsqrt_rn(a * a + b * b) : 0.0;
        }
        lds[r * pitch + q] = d;
        q += dq;
        r += dr;
        if (r >= D) {
            r -= D;
            ++q;
        }
    }
    __syncthreads();

    // lane j's output: one chain over the taps ascending, from +0.0
    if (tid < n_tile) {
        const char *base = reinterpret_cast<const char *>(lds + tid);
        double acc = 0.0;
        int k = 0;
        for (; k + 8 <= L; k += 8) {
            double x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const double *>(base + offs[k + j]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = acc + taps[k + j] * x[j];
        }
        for (; k < L; ++k) acc = acc + taps[k] * *reinterpret_cast<const double *>(base + offs[k]);
        audio[out_first + (unsigned)(i0 + tid)] = (float)(gain * acc);
    }
}

struct fsea_audio {
    int kind = 0;         // the four plain numbers first: the checks of a run read `decimation` and nothing else
    int n_taps = 0;
    int decimation = 1;
    int device = 0;
    int tile = 0, pitch = 0;                       // audio_tile, audio_pitch
    fsea_detail::DeviceArray<double> d_taps;       // n_taps doubles
    fsea_detail::DeviceArray<uint32_t> d_offs;     // n_taps byte offsets of the taps' values in the LDS image
    fsea_detail::JobTable table;                   // the jobs and their first-tile column
    std::mutex mu;
    fsea_detail::HostStaging staging;              // the host form
};
static_assert(offsetof(fsea_audio, kind) == 0 && offsetof(fsea_audio, n_taps) == 4 && offsetof(fsea_audio, decimation) == 8 &&
              offsetof(fsea_audio, device) == 12, "the fake object of tests/test_audio_host.py");

namespace {

// where job i's audio lies, (out_first, count): the placement check's, the layout's and the host form's
auto placed(const fsea_audio *a, const fsea_audio_job *jobs) {
    return [a, jobs](size_t i, uint64_t *first, uint64_t *n) {
        *first = jobs[i].out_first;
        *n = jobs[i].n_pairs / (uint64_t)a->decimation;
    };
}

// Everything a run checks but the alignment, in the header's order, reading nothing of the object but its decimation.
int check_run(const fsea_audio *a, const void *pairs, size_t n_buffer_pairs, const fsea_audio_job *jobs, size_t n_jobs,
              double offset_re, double offset_im, double gain, const void *audio, size_t n_audio) {
    if (int rc = fsea_detail::check_jobs_head(a, "audio", n_jobs, jobs, pairs, audio)) return rc;
    if (n_jobs == 0) return FSEA_OK;
    if (int rc = fsea_detail::check_offset(offset_re, offset_im)) return rc;
    if (!std::isfinite(gain)) return fail(FSEA_EINVAL, "the gain is not finite");
    uint64_t total = 0;
    const int rc = fsea_detail::check_jobs_placement(n_jobs, n_audio, "", " of the audio", [&](size_t i, uint64_t *first, uint64_t *n) {
        const fsea_audio_job &j = jobs[i];
        placed(a, jobs)(i, first, n);
        total += *n;
        return fsea_detail::check_job_span(i, j.first_pair, j.n_pairs, n_buffer_pairs, FSEA_AUDIO_MAX_PAIRS, "pairs", "buffer");
    });
    if (rc) return rc;
    return fsea_detail::check_jobs_total(total, "outputs");
}

// One call on device buffers, asynchronous on `s`: the table built in mapped host memory, its upload, the launch.  The
// caller holds a->mu and is on a's device; the arguments are checked and n_jobs is at least 1.
int queue_call(fsea_audio *a, const void *d_pairs, const fsea_audio_job *jobs, size_t n_jobs, double offset_re, double offset_im,
               double gain, float *d_audio, hipStream_t s) {
    const uint64_t D = (uint64_t)a->decimation;
    uint64_t tiles = 0;
    for (size_t i = 0; i < n_jobs; ++i) tiles += (jobs[i].n_pairs / D + (unsigned)a->tile - 1) / (unsigned)a->tile;
    if (tiles == 0) return FSEA_OK;
    fsea_detail::JobTable::Built<fsea_audio_job> t;
    const int rc = a->table.build<fsea_audio_job>(n_jobs, (unsigned)a->tile, 0, s, [&](size_t i, fsea_audio_job &rec, uint32_t) {
        rec = jobs[i];
        return jobs[i].n_pairs / D;
    }, &t);
    if (rc) return rc;
    hipLaunchKernelGGL(fsea_audio_tiles, dim3((unsigned)t.tiles), dim3(AU_WG), 0, s, static_cast<const float2 *>(d_pairs), t.recs, t.tile0,
                       (int)n_jobs, fsea_detail::job_steps(n_jobs), a->kind, (const double *)a->d_taps.ptr, (const uint32_t *)a->d_offs.ptr,
                       a->n_taps, a->decimation, a->tile, a->pitch, offset_re, offset_im, gain, d_audio);
    FSEA_HIP(hipGetLastError());
    return a->table.release(s);
}

}  // namespace

extern "C" {

int fsea_audio_create(fsea_audio **out, int kind, const double *taps, int n_taps, int decimation, int device) {
    if (!out) return fail(FSEA_EINVAL, "audio out-pointer is NULL");
    *out = nullptr;
    if (kind != FSEA_AUDIO_FM && kind != FSEA_AUDIO_AM) return fail(FSEA_EINVAL, "kind must be FSEA_AUDIO_FM or FSEA_AUDIO_AM, got %d", kind);
    if (int rc = fsea_stage::FirState::check_taps(taps, n_taps)) return rc;
    if (decimation < 1 || decimation > FSEA_AUDIO_MAX_DECIMATION) {
        return fail(FSEA_EINVAL, "decimation must be in [1, %d], got %d", FSEA_AUDIO_MAX_DECIMATION, decimation);
    }
    return fsea_detail::create_object(out, device, "fsea_audio_create", [&](fsea_audio *a) -> hipError_t {
        a->kind = kind;
        a->n_taps = n_taps;
        a->decimation = decimation;
        a->tile = audio_tile(decimation, n_taps);
        a->pitch = audio_pitch(decimation, n_taps);
        uint32_t offs[FSEA_FIR_MAX_TAPS];
        for (int k = 0; k < n_taps; ++k) offs[k] = (uint32_t)(((k % decimation) * a->pitch + k / decimation) * (int)sizeof(double));
        hipError_t e = a->d_taps.upload(taps, (size_t)n_taps);
        if (e == hipSuccess) e = a->d_offs.upload(offs, (size_t)n_taps);
        if (e == hipSuccess) e = a->table.create(a->staging.stream);
        return e;
    });
}

int fsea_audio_destroy(fsea_audio *a) { return fsea_detail::destroy_object(a); }

int fsea_audio_kind(const fsea_audio *a) { return a ? a->kind : -1; }

int fsea_audio_decimation(const fsea_audio *a) { return a ? a->decimation : 0; }

int fsea_audio_n_taps(const fsea_audio *a) { return a ? a->n_taps : 0; }

int fsea_audio_layout(const fsea_audio *a, fsea_audio_job *jobs, size_t n_jobs, size_t *total_outputs) {
    return fsea_detail::layout_jobs(a, "audio", jobs, n_jobs, total_outputs, "total_outputs", 1, placed(a, jobs));
}

int fsea_audio_run_device(fsea_audio *a, const void *d_pairs, size_t n_buffer_pairs, const fsea_audio_job *jobs, size_t n_jobs,
                          double offset_re, double offset_im, double gain, float *d_audio, size_t n_audio, void *stream) {
    const int rc = check_run(a, d_pairs, n_buffer_pairs, jobs, n_jobs, offset_re, offset_im, gain, d_audio, n_audio);
    if (rc || n_jobs == 0) return rc;
    return fsea_detail::run_device_pairs(a, d_pairs, d_audio, "d_audio", 4, stream, [&](hipStream_t s) {
        return queue_call(a, d_pairs, jobs, n_jobs, offset_re, offset_im, gain, d_audio, s);
    });
}

int fsea_audio_run_host(fsea_audio *a, const float *pairs, size_t n_buffer_pairs, const fsea_audio_job *jobs, size_t n_jobs,
                        double offset_re, double offset_im, double gain, float *audio, size_t n_audio) {
    const int rc = check_run(a, pairs, n_buffer_pairs, jobs, n_jobs, offset_re, offset_im, gain, audio, n_audio);
    if (rc || n_jobs == 0) return rc;
    const uint64_t D = (uint64_t)a->decimation;
    const size_t end_in = fsea_detail::staged_pairs(jobs, n_jobs, [D](const fsea_audio_job &j) { return j.n_pairs / D != 0; });
    return fsea_detail::run_host_placed(
        a, end_in * sizeof(float2), n_jobs, audio, [&](void *h_in) { std::memcpy(h_in, pairs, end_in * sizeof(float2)); },
        [&](void *d_in, float *d_out, hipStream_t s) { return queue_call(a, d_in, jobs, n_jobs, offset_re, offset_im, gain, d_out, s); },
        placed(a, jobs));
}

}  // extern "C"
