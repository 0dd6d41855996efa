// fsea_spectra.hip -- cut-out spectra (include/fsea.h: fsea_spectra_*): a table of jobs over one resident buffer of f32 pairs,
// one averaged periodogram of n bins per job -- of the cut-out itself, of its envelope |z|^2, of z^2 or of z^4 -- in one launch
// for the tiles and one for the fold.  fsea_extract turns each box into its signal, fsea_measure says what is inside,
// fsea_audio what it carries; this says what it looks like in frequency, and the three nonlinear kinds say what kind of
// emission it is.  No state between calls.  The terms, the kinds, the taper and the sign are f32 with the roundings the
// header writes out; the transform's own roundings are this file's; the average is f64 in an order the header fixes, so a
// job's n floats are a function of its pairs alone, bit for bit.
//
// Kernel fsea_spectra_tiles_<n> ("Cut-out spectra"): one workgroup of SP_WG = 256 lanes per tile of
// FSEA_SPECTRA_TILE_SEGMENTS segments of one job; the grid is the sum of the jobs' tiles.  The device table is the caller's
// jobs as they are and a column of first tiles, built and brought there as the others' (fsea_jobs.h: JobTable), the
// tiles' partials behind it; a workgroup finds its job by job_of_tile, scalar loads.  A round transforms G = max(1, 1024 / n)
// segments at once, P = G n = max(n, 1024) points, so that all 256 lanes have a radix-4 butterfly in every pass at any n.
// The transform is Stockham's autosort, radix 4 with a final radix 2 where log2 n is odd, from one template on log2 n: pass 0
// takes its inputs from global memory -- lane j's four are the pairs j, j + n / 4, j + n / 2, j + 3 n / 4 of the segment,
// 8-byte loads, a wave's 64 of them 512 contiguous bytes at any parity of first_pair -- and makes term, kind, taper and
// sign of each on the way; every later pass goes from one LDS image to the other, one barrier a pass.  The twiddles are
// the object's table of n f32 pairs, e^(-2 pi i m / n) computed in f64.  Behind the last pass lane l adds the powers of bins
// l, l + 256, ... of the round's segments, ascending, to f64 accumulators it keeps in registers over the tile's rounds, and
// stores them as the tile's partial, 8 bytes a lane.  Kernel fsea_spectra_fold: a workgroup per job and 256 bins adds the
// job's partials in tile order, divides and stores.  No atomics, no wave waits for another but at the barriers, every loop
// has its bound on entry.
#include "fsea_jobs.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

// every product and sum below is rounded on its own: a a + b b, w u and the butterflies' products must not become an FMA
#pragma clang fp contract(off)

using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int SP_WG = 256;
constexpr int SP_TILE = FSEA_SPECTRA_TILE_SEGMENTS;
constexpr int SP_ROUND = 1024;                                // points a round transforms at the least: four a lane
static_assert(sizeof(fsea_spectra_job) == 24, "the record of include/fsea.h");
static_assert(FSEA_SPECTRA_MIN_N == 64 && FSEA_SPECTRA_MAX_N == 4096 && FSEA_SPECTRA_MIN_N / 4 >= 2, "(-1)^j is one sign for a lane's four inputs");

// the geometry of one size
template <int LOG2N>
struct Geo {
    static constexpr int N = 1 << LOG2N;
    static constexpr int G = N >= SP_ROUND ? 1 : SP_ROUND / N;       // segments a round
    static constexpr int P = G * N;                                     // points a round
    static constexpr int B4 = P / 4 / SP_WG;                            // radix-4 butterflies a lane and pass
    static constexpr int B2 = P / 2 / SP_WG;                            // radix-2 butterflies a lane in the last pass of an odd log2 n
    static constexpr int PASSES4 = LOG2N / 2;
    static constexpr bool ODD = (LOG2N & 1) != 0;
    static constexpr int PASSES = PASSES4 + (ODD ? 1 : 0);
    static constexpr int ACC = N >= SP_WG ? N / SP_WG : 1;             // bins a lane accumulates
    static_assert(SP_TILE % G == 0, "a tile is whole rounds");
};

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// what pass 0 needs to make an input of a pair
struct Terms {
    double off_re, off_im;
    int kind;
    const float *__restrict__ window;   // n weights or null
};

// the header's input x_j of the pair z, j its place in the segment: term, kind, taper, sign
__device__ __forceinline__ float2 input_of(const Terms &t, float2 z, unsigned j) {
    const float a = (float)((double)z.x - t.off_re), b = (float)((double)z.y - t.off_im);
    float u = a, v = b;
    if (t.kind == FSEA_SPECTRA_ENVELOPE) {
        u = a * a + b * b;
        v = 0.0f;
    } else if (t.kind != FSEA_SPECTRA_Z) {
        u = a * a - b * b;
        v = 2.0f * (a * b);
        if (t.kind == FSEA_SPECTRA_FOURTH) {
            const float u1 = u, v1 = v;
            u = u1 * u1 - v1 * v1;
            v = 2.0f * (u1 * v1);
        }
    }
    if (t.window) {
        const float w = t.window[j];
        u = w * u;
        v = w * v;
    }
    return (j & 1u) ? make_float2(-u, -v) : make_float2(u, v);
}

// one radix-4 butterfly of the pass whose sub-transforms have ns points so far: v[r] is input j + r n / 4 of the segment;
// the outputs go to out[j0 + r ns], j0 = 4 (j - k) + k, k = j mod ns.  tw: e^(-2 pi i m / n), m < n.
template <int N>
__device__ __forceinline__ void butterfly4(float2 (&v)[4], unsigned j, unsigned ns, const float2 *__restrict__ tw, float2 *__restrict__ out) {
    const unsigned k = j & (ns - 1u);
    if (ns > 1u) {                        // the first pass has k = 0: no twiddle
        const unsigned step = (unsigned)N / (4u * ns);
        v[1] = cmul(v[1], tw[k * step]);
        v[2] = cmul(v[2], tw[2u * k * step]);
        v[3] = cmul(v[3], tw[3u * k * step]);
    }
    const float2 s0 = cadd(v[0], v[2]), s1 = csub(v[0], v[2]), s2 = cadd(v[1], v[3]), s3 = csub(v[1], v[3]);
    const float2 m3 = make_float2(s3.y, -s3.x);   // -i s3
    const unsigned j0 = ((j - k) << 2) + k;
    out[j0] = cadd(s0, s2);
    out[j0 + ns] = cadd(s1, m3);
    out[j0 + 2u * ns] = csub(s0, s2);
    out[j0 + 3u * ns] = csub(s1, m3);
}

// The tile `tile` of the call: its job's segments seg0 .. seg0 + n_seg - 1, n_seg <= SP_TILE, every one inside the job.
template <int LOG2N>
__device__ __forceinline__ void spectra_tile(const float2 *__restrict__ pairs, const fsea_spectra_job *__restrict__ jobs,
                                             const uint32_t *__restrict__ tile0, int n_jobs, int steps, int hop, Terms terms,
                                             const float2 *__restrict__ tw, double *__restrict__ partials, float2 *lds) {
    using g = Geo<LOG2N>;
    constexpr unsigned N = g::N, T4 = N / 4, T2 = N / 2;
    const unsigned tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;

    const int lo = fsea_detail::job_of_tile(tile0, n_jobs, steps, tile);
    const unsigned long long first = jobs[lo].first_pair;
    const unsigned n_pairs = (unsigned)jobs[lo].n_pairs;                    // <= 2^24, and >= N: the job has a tile
    const unsigned S = (n_pairs - N) / (unsigned)hop + 1u;
    const unsigned seg0 = (tile - tile0[lo]) * (unsigned)SP_TILE;           // below S
    const unsigned left = S - seg0;
    const unsigned n_seg = left < (unsigned)SP_TILE ? left : (unsigned)SP_TILE;
    const float2 *__restrict__ job = pairs + first;

    float2 *bufs[2] = {lds, lds + g::P};
    double acc[g::ACC];
#pragma unroll
    for (int c = 0; c < g::ACC; ++c) acc[c] = 0.0;

    for (unsigned r0 = 0; r0 < n_seg; r0 += (unsigned)g::G) {               // a round: segments seg0 + r0 .. + G - 1
        const unsigned here = n_seg - r0 < (unsigned)g::G ? n_seg - r0 : (unsigned)g::G;
        // pass 0, from global memory.  A pair read is s hop + j + r n / 4 < (S - 1) hop + n <= n_pairs of the job
        {
            float2 v[g::B4][4];
#pragma unroll
            for (int q = 0; q < g::B4; ++q) {
                const unsigned t = tid + (unsigned)SP_WG * q, sg = t / T4, j = t - sg * T4;
                const float2 *__restrict__ seg = job + (size_t)(seg0 + r0 + sg) * (unsigned)hop;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[q][r] = sg < here ? seg[j + r * T4] : make_float2(0.0f, 0.0f);
            }
#pragma unroll
            for (int q = 0; q < g::B4; ++q) {
                const unsigned t = tid + (unsigned)SP_WG * q, sg = t / T4, j = t - sg * T4;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[q][r] = input_of(terms, v[q][r], j + r * T4);
                butterfly4<N>(v[q], j, 1u, tw, bufs[0] + sg * N);
            }
        }
        __syncthreads();
        // the radix-4 passes 1 .. PASSES4 - 1, image to image
        unsigned ns = 4;
#pragma unroll
        for (int p = 1; p < g::PASSES4; ++p) {
            const float2 *in = bufs[(p - 1) & 1];
            float2 *out = bufs[p & 1];
#pragma unroll
            for (int q = 0; q < g::B4; ++q) {
                const unsigned t = tid + (unsigned)SP_WG * q, sg = t / T4, j = t - sg * T4;
                float2 v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = in[sg * N + j + r * T4];
                butterfly4<N>(v, j, ns, tw, out + sg * N);
            }
            ns <<= 2;
            __syncthreads();
        }
        if (g::ODD) {                                                       // the radix-2 pass: ns = n / 2, k = j
            const float2 *in = bufs[(g::PASSES4 - 1) & 1];
            float2 *out = bufs[g::PASSES4 & 1];
#pragma unroll
            for (int q = 0; q < g::B2; ++q) {
                const unsigned t = tid + (unsigned)SP_WG * q, sg = t / T2, j = t - sg * T2;
                const float2 a = in[sg * N + j], b = cmul(in[sg * N + j + T2], tw[j]);
                out[sg * N + j] = cadd(a, b);
                out[sg * N + j + T2] = csub(a, b);
            }
            __syncthreads();
        }
        // the round's powers to the lane's bins, segments ascending
        const float2 *X = bufs[(g::PASSES - 1) & 1];
#pragma unroll
        for (int c = 0; c < g::ACC; ++c) {
            const unsigned bin = tid + (unsigned)SP_WG * c;
            if (bin < N) {
                for (unsigned sg = 0; sg < here; ++sg) {
                    const float2 x = X[sg * N + bin];
                    acc[c] = acc[c] + (double)(x.x * x.x + x.y * x.y);
                }
            }
        }
        __syncthreads();                                                   // the next round writes both images
    }
    double *__restrict__ mine = partials + (size_t)tile * N;
#pragma unroll
    for (int c = 0; c < g::ACC; ++c) {
        const unsigned bin = tid + (unsigned)SP_WG * c;
        if (bin < N) mine[bin] = acc[c];
    }
}

}  // namespace

// grid: the tiles of all jobs; tile0[k] is job k's first tile, a job's tiles follow one another; partials: n doubles a tile
#define FSEA_SPECTRA_TILES_(LOG2N, NPOINTS)                                                                                       \
    extern "C" __global__ __launch_bounds__(SP_WG) void fsea_spectra_tiles_##NPOINTS(                                             \
        const float2 *__restrict__ pairs, const fsea_spectra_job *__restrict__ jobs, const uint32_t *__restrict__ tile0, int n_jobs, \
        int steps, int hop, int kind, const float *__restrict__ window, const float2 *__restrict__ tw, double off_re, double off_im, \
        double *__restrict__ partials) {                                                                                          \
        __shared__ __attribute__((aligned(16))) float2 lds[2 * Geo<LOG2N>::P];                                                   \
        spectra_tile<LOG2N>(pairs, jobs, tile0, n_jobs, steps, hop, Terms{off_re, off_im, kind, window}, tw, partials, lds);      \
    }
FSEA_SPECTRA_TILES_(6, 64)
FSEA_SPECTRA_TILES_(7, 128)
FSEA_SPECTRA_TILES_(8, 256)
FSEA_SPECTRA_TILES_(9, 512)
FSEA_SPECTRA_TILES_(10, 1024)
FSEA_SPECTRA_TILES_(11, 2048)
FSEA_SPECTRA_TILES_(12, 4096)

// grid: chunks = max(1, n / 256) workgroups a job, job after job; a job without a segment stores nothing
extern "C" __global__ __launch_bounds__(SP_WG) void fsea_spectra_fold(const fsea_spectra_job *__restrict__ jobs,
                                                                     const uint32_t *__restrict__ tile0,
                                                                     const double *__restrict__ partials, int n, int hop, int chunks,
                                                                     float *__restrict__ power) {
    const uint32_t k = blockIdx.x / (unsigned)chunks;
    const unsigned bin = (blockIdx.x - k * (unsigned)chunks) * (unsigned)SP_WG + threadIdx.x;
    const unsigned n_pairs = (unsigned)jobs[k].n_pairs;
    if (n_pairs < (unsigned)n || bin >= (unsigned)n) return;
    const unsigned S = (n_pairs - (unsigned)n) / (unsigned)hop + 1u;
    const unsigned tiles = (S + (unsigned)SP_TILE - 1u) / (unsigned)SP_TILE;
    const double *__restrict__ mine = partials + (size_t)tile0[k] * (unsigned)n + bin;
    double sum = 0.0;
    for (unsigned t = 0; t < tiles; ++t) sum = sum + mine[(size_t)t * (unsigned)n];
    power[jobs[k].out_first + bin] = (float)__ddiv_rn(sum, (double)S);
}

struct fsea_spectra {
    int n = 0;            // the four plain numbers first: the checks of a run read n and hop and nothing else
    int hop = 0;
    int kind = 0;
    int device = 0;
    bool tapered = false;
    fsea_detail::DeviceArray<float> d_window;      // n weights, with a taper
    fsea_detail::DeviceArray<float2> d_tw;         // e^(-2 pi i m / n), m < n
    fsea_detail::JobTable table;                   // the jobs and their first-tile column; behind them, the tiles' partials
    std::mutex mu;
    fsea_detail::HostStaging staging;              // the host form
};
static_assert(offsetof(fsea_spectra, n) == 0 && offsetof(fsea_spectra, hop) == 4 && offsetof(fsea_spectra, kind) == 8 &&
              offsetof(fsea_spectra, device) == 12, "the fake object of tests/test_spectra_host.py");

namespace {

bool size_ok(int n) { return n >= FSEA_SPECTRA_MIN_N && n <= FSEA_SPECTRA_MAX_N && (n & (n - 1)) == 0; }

// S of the header
uint64_t segments_of(uint64_t n_pairs, int n, int hop) { return n_pairs < (uint64_t)n ? 0 : (n_pairs - (uint64_t)n) / (uint64_t)hop + 1; }

// where job i's powers lie: (out_first, count): the placement check's, the layout's and the host form's
auto placed(const fsea_spectra *sp, const fsea_spectra_job *jobs) {
    return [sp, jobs](size_t i, uint64_t *first, uint64_t *count) {
        *first = jobs[i].out_first;
        *count = segments_of(jobs[i].n_pairs, sp->n, sp->hop) ? (uint64_t)sp->n : 0;
    };
}

// Everything a run checks but the alignment, in the header's order, reading nothing of the object but n and hop.
int check_run(const fsea_spectra *sp, const void *pairs, size_t n_buffer_pairs, const fsea_spectra_job *jobs, size_t n_jobs,
              double offset_re, double offset_im, const void *power, size_t n_power) {
    if (int rc = fsea_detail::check_jobs_head(sp, "spectra", n_jobs, jobs, pairs, power)) return rc;
    if (n_jobs == 0) return FSEA_OK;
    if (int rc = fsea_detail::check_offset(offset_re, offset_im)) return rc;
    const int n = sp->n, hop = sp->hop;
    uint64_t total = 0;
    const int rc = fsea_detail::check_jobs_placement(n_jobs, n_power, "", " of the power", [&](size_t i, uint64_t *first, uint64_t *count) {
        const fsea_spectra_job &j = jobs[i];
        const uint64_t S = segments_of(j.n_pairs, n, hop);
        placed(sp, jobs)(i, first, count);
        total += S <= ((uint64_t)1 << 32) ? S * (uint64_t)n : (uint64_t)1 << 44;   // a span that is refused anyway
        return fsea_detail::check_job_span(i, j.first_pair, j.n_pairs, n_buffer_pairs, FSEA_SPECTRA_MAX_PAIRS, "pairs", "buffer");
    });
    if (rc) return rc;
    return fsea_detail::check_jobs_total(total, "points");
}

const void *tiles_kernel(int n) {
    switch (n) {
    case 64: return reinterpret_cast<const void *>(&fsea_spectra_tiles_64);
    case 128: return reinterpret_cast<const void *>(&fsea_spectra_tiles_128);
    case 256: return reinterpret_cast<const void *>(&fsea_spectra_tiles_256);
    case 512: return reinterpret_cast<const void *>(&fsea_spectra_tiles_512);
    case 1024: return reinterpret_cast<const void *>(&fsea_spectra_tiles_1024);
    case 2048: return reinterpret_cast<const void *>(&fsea_spectra_tiles_2048);
    default: return reinterpret_cast<const void *>(&fsea_spectra_tiles_4096);
    }
}

// One call on device buffers, asynchronous on `s`: the table built in mapped host memory, its upload, the tiles, the fold.
// The caller holds sp->mu and is on sp's device; the arguments are checked and n_jobs is at least 1.
int queue_call(fsea_spectra *sp, const void *d_pairs, const fsea_spectra_job *jobs, size_t n_jobs, double offset_re, double offset_im,
               float *d_power, hipStream_t s) {
    const int n = sp->n, hop = sp->hop;
    uint64_t tiles = 0;
    for (size_t i = 0; i < n_jobs; ++i) tiles += (segments_of(jobs[i].n_pairs, n, hop) + SP_TILE - 1) / SP_TILE;
    if (tiles == 0) return FSEA_OK;
    fsea_detail::JobTable::Built<fsea_spectra_job> t;
    const int rc = sp->table.build<fsea_spectra_job>(n_jobs, SP_TILE, sizeof(double) * (size_t)n, s, [&](size_t i, fsea_spectra_job &rec, uint32_t) {
        rec = jobs[i];
        return segments_of(jobs[i].n_pairs, n, hop);
    }, &t);
    if (rc) return rc;
    const float2 *pairs = static_cast<const float2 *>(d_pairs);
    const fsea_spectra_job *recs = t.recs;
    const uint32_t *tile0 = t.tile0;
    int jobs_i = (int)n_jobs, steps = fsea_detail::job_steps(n_jobs), hop_i = hop, kind = sp->kind, n_i = n;
    const float *window = sp->tapered ? sp->d_window.ptr : nullptr;
    const float2 *tw = sp->d_tw.ptr;
    double *partials = reinterpret_cast<double *>(t.behind);
    void *args[] = {&pairs, &recs, &tile0, &jobs_i, &steps, &hop_i, &kind, &window, &tw, &offset_re, &offset_im, &partials};
    FSEA_HIP(hipLaunchKernel(tiles_kernel(n), dim3((unsigned)t.tiles), dim3(SP_WG), args, 0, s));
    int chunks = n >= SP_WG ? n / SP_WG : 1;
    hipLaunchKernelGGL(fsea_spectra_fold, dim3((unsigned)(n_jobs * (size_t)chunks)), dim3(SP_WG), 0, s, recs, tile0,
                       static_cast<const double *>(partials), n_i, hop_i, chunks, d_power);
    FSEA_HIP(hipGetLastError());
    return sp->table.release(s);
}

}  // namespace

extern "C" {

int fsea_spectra_create(fsea_spectra **out, int n, int hop, int kind, const float *window, int device) {
    if (!out) return fail(FSEA_EINVAL, "spectra out-pointer is NULL");
    *out = nullptr;
    if (!size_ok(n)) return fail(FSEA_EINVAL, "n must be a power of two in [%d, %d], got %d", FSEA_SPECTRA_MIN_N, FSEA_SPECTRA_MAX_N, n);
    if (hop < 1 || hop > n) return fail(FSEA_EINVAL, "hop must be in [1, %d], got %d", n, hop);
    if (kind < FSEA_SPECTRA_Z || kind > FSEA_SPECTRA_FOURTH) {
        return fail(FSEA_EINVAL, "kind must be FSEA_SPECTRA_Z, _ENVELOPE, _SQUARE or _FOURTH, got %d", kind);
    }
    for (int j = 0; window && j < n; ++j) {
        if (!std::isfinite(window[j])) return fail(FSEA_EINVAL, "window weight %d is not finite", j);
    }
    return fsea_detail::create_object(out, device, "fsea_spectra_create", [&](fsea_spectra *sp) -> hipError_t {
        sp->n = n;
        sp->hop = hop;
        sp->kind = kind;
        sp->tapered = window != nullptr;
        std::vector<float2> tw((size_t)n);
        for (int m = 0; m < n; ++m) {
            const double a = -2.0 * M_PI * (double)m / (double)n;
            tw[(size_t)m] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        // the quarter turns exactly: cos and sin of a rounded multiple of pi leave 6e-17 where 0 belongs
        tw[0] = make_float2(1.0f, 0.0f);
        tw[(size_t)n / 4] = make_float2(0.0f, -1.0f);
        tw[(size_t)n / 2] = make_float2(-1.0f, 0.0f);
        tw[(size_t)(3 * n / 4)] = make_float2(0.0f, 1.0f);
        hipError_t e = sp->d_tw.upload(tw.data(), (size_t)n);
        if (e == hipSuccess && window) e = sp->d_window.upload(window, (size_t)n);
        if (e == hipSuccess) e = sp->table.create(sp->staging.stream);
        return e;
    });
}

int fsea_spectra_destroy(fsea_spectra *sp) { return fsea_detail::destroy_object(sp); }

int fsea_spectra_n(const fsea_spectra *sp) { return sp ? sp->n : 0; }

int fsea_spectra_hop(const fsea_spectra *sp) { return sp ? sp->hop : 0; }

int fsea_spectra_kind(const fsea_spectra *sp) { return sp ? sp->kind : -1; }

size_t fsea_spectra_segments(const fsea_spectra *sp, size_t n_pairs) { return sp ? (size_t)segments_of(n_pairs, sp->n, sp->hop) : 0; }

int fsea_spectra_layout(const fsea_spectra *sp, fsea_spectra_job *jobs, size_t n_jobs, size_t *total_floats) {
    return fsea_detail::layout_jobs(sp, "spectra", jobs, n_jobs, total_floats, "total_floats", 1, placed(sp, jobs));
}

int fsea_spectra_run_device(fsea_spectra *sp, const void *d_pairs, size_t n_buffer_pairs, const fsea_spectra_job *jobs, size_t n_jobs,
                            double offset_re, double offset_im, float *d_power, size_t n_power, void *stream) {
    const int rc = check_run(sp, d_pairs, n_buffer_pairs, jobs, n_jobs, offset_re, offset_im, d_power, n_power);
    if (rc || n_jobs == 0) return rc;
    return fsea_detail::run_device_pairs(sp, d_pairs, d_power, "d_power", 4, stream, [&](hipStream_t s) {
        return queue_call(sp, d_pairs, jobs, n_jobs, offset_re, offset_im, d_power, s);
    });
}

int fsea_spectra_run_host(fsea_spectra *sp, const float *pairs, size_t n_buffer_pairs, const fsea_spectra_job *jobs, size_t n_jobs,
                          double offset_re, double offset_im, float *power, size_t n_power) {
    const int rc = check_run(sp, pairs, n_buffer_pairs, jobs, n_jobs, offset_re, offset_im, power, n_power);
    if (rc || n_jobs == 0) return rc;
    const size_t end_in = fsea_detail::staged_pairs(
        jobs, n_jobs, [sp](const fsea_spectra_job &j) { return segments_of(j.n_pairs, sp->n, sp->hop) != 0; });
    return fsea_detail::run_host_placed(
        sp, end_in * sizeof(float2), n_jobs, power, [&](void *h_in) { std::memcpy(h_in, pairs, end_in * sizeof(float2)); },
        [&](void *d_in, float *d_out, hipStream_t s) { return queue_call(sp, d_in, jobs, n_jobs, offset_re, offset_im, d_out, s); },
        placed(sp, jobs));
}

int fsea_spectra_jobs(const fsea_extract_job *ejobs, size_t n_jobs, int decimation, size_t skip_pairs, fsea_spectra_job *jobs) {
    return fsea_detail::jobs_of_extract(ejobs, n_jobs, decimation, skip_pairs, FSEA_SPECTRA_MAX_PAIRS, jobs,
                                        [](fsea_spectra_job &j) { j.out_first = 0; });   // fsea_spectra_layout places them
}

// Host arithmetic; no device is touched.  Each line is the header's formula; 0 / 0 gives the NaN of a silent row.
int fsea_spectra_finish(const float *power, int n, int guard_bins, double fraction, fsea_spectra_result *result) {
    if (!power || !result) return fail(FSEA_EINVAL, "NULL buffer");
    if (!size_ok(n)) return fail(FSEA_EINVAL, "n must be a power of two in [%d, %d], got %d", FSEA_SPECTRA_MIN_N, FSEA_SPECTRA_MAX_N, n);
    if (guard_bins < -1 || guard_bins > n / 2 - 1) return fail(FSEA_EINVAL, "guard_bins must be in [-1, %d], got %d", n / 2 - 1, guard_bins);
    if (!(fraction > 0.0 && fraction <= 1.0)) return fail(FSEA_EINVAL, "fraction must be in (0, 1]");
    const int half = n / 2;
    const double nan = std::nan("");
    fsea_spectra_result r;
    double total = 0.0, moment = 0.0;
    for (int k = 0; k < n; ++k) {
        total += (double)power[k];
        moment += (double)(k - half) * (double)power[k];
    }
    r.total = total;
    r.centroid_cycles = moment / total / (double)n;
    // the occupied band: the least k whose running sum is above t, the least whose running sum reaches total - t
    const double t = total * (1.0 - fraction) / 2.0;
    double c = 0.0;
    r.obw_lo = r.obw_hi = -1;
    for (int k = 0; k < n; ++k) {
        c += (double)power[k];
        if (r.obw_lo < 0 && c > t) r.obw_lo = k;
        if (r.obw_hi < 0 && c >= total - t) r.obw_hi = k;
    }
    const bool band = r.obw_lo >= 0 && r.obw_hi >= 0;
    if (!band) r.obw_lo = r.obw_hi = -1;
    r.obw_bins = band ? r.obw_hi - r.obw_lo + 1 : 0;
    r.obw_centre_cycles = band ? ((double)(r.obw_lo + r.obw_hi) / 2.0 - (double)half) / (double)n : nan;
    // the strongest line outside the guard and the lower median of the same bins
    std::vector<float> rest;
    rest.reserve((size_t)n);
    r.peak_bin = -1;
    float peak = 0.0f;
    for (int k = 0; k < n; ++k) {
        if (std::abs(k - half) <= guard_bins) continue;
        if (r.peak_bin < 0 || power[k] > peak) {
            peak = power[k];
            r.peak_bin = k;
        }
        rest.push_back(power[k]);
    }
    std::nth_element(rest.begin(), rest.begin() + (std::ptrdiff_t)((rest.size() - 1) / 2), rest.end(),
                     [](float a, float b) { return a < b || (b != b && a == a); });   // a total order: NaN behind everything
    r.peak_power = (double)peak;
    r.peak_cycles = (double)(r.peak_bin - half) / (double)n;
    r.floor = (double)rest[(rest.size() - 1) / 2];
    r.line_db = 10.0 * std::log10(r.peak_power / r.floor);
    *result = r;
    return FSEA_OK;
}

}  // extern "C"
