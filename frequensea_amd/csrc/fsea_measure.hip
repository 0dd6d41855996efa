// fsea_measure.hip -- signal measures (include/fsea.h: fsea_measure_*): a table of jobs over one resident buffer of f32 pairs,
// one record of moment sums per job -- sum z, sum |z|^2, sum |z|^4, the lag product sum z[i] conj(z[i - lag]) and the largest
// |z|^2 with its place -- in one launch for the tiles and one for the fold.  fsea_extract turns each box into its signal;
// this says what is inside.  No state between calls.  The sums are f64 in an order the header fixes term by term (fold_256
// inside a tile, fold_64 over a job's tiles), so a job's record is a function of its pairs alone, bit for bit.
//
// Kernel fsea_measure_tiles ("Signal measures"): one workgroup of MS_WG = 256 lanes per tile of
// MS_TILE = 4096 pairs of one job; the grid is the sum of the jobs' tiles.  The device table is the caller's jobs as they are
// and a column of first tiles, built and brought there as fsea_extract's and fsea_audio's (fsea_jobs.h: JobTable::build),
// the tile partials behind it; a workgroup finds its job by a bisection over that column (job_of_tile), `steps` =
// ceil(log2(jobs)) <= 16 loads, uniform, so scalar loads and SGPRs, and so is the job itself.  A job without pairs has
// its successor's first tile and the bisection ends at the last job whose first tile is not behind the workgroup's:
// never at an empty one.  Lane l takes pairs l, l + 256, ... of the tile: sixteen 8-byte loads, a wave's 64 of them
// 512 contiguous bytes at any parity of first_pair, and sixteen more for the lagged partners (the same lines `lag` pairs
// earlier, cache hits), all issued in front of the arithmetic.  A tile that is whole and has a partner for every pair takes a body without bounds tests; the
// other body tests every pair and does the same operations in the same order.  Six f64 accumulators, the running maximum
// and its index stay in registers; the 256-lane combine is the xor butterfly across a wave's lanes (k = 1 .. 32) and the
// last two stages (k = 64, 128) over the four waves' values in LDS; lanes 0 .. 7 store the tile's partial, 8 bytes each.
// Kernel fsea_measure_fold: one wave per job runs fold_64 over the job's partials and stores the 80-byte record.  No float
// atomics, no wave waits for another, every loop has its bound on entry.
#include "fsea_jobs.h"

#include <algorithm>
#include <cmath>

// every product and sum below is rounded on its own: P P + q, a a + b b and the like must not become one FMA
#pragma clang fp contract(off)

using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int MS_WG = 256;
constexpr int MS_TILE = FSEA_MEASURE_TILE_PAIRS;
constexpr int MS_STEPS = MS_TILE / MS_WG;   // pairs per lane and tile
static_assert(MS_STEPS == 16 && MS_WG == 4 * 64, "fold_256: four waves, sixteen pairs a lane");
static_assert(sizeof(fsea_measure_job) == 16 && sizeof(fsea_measure_sums) == 80, "the records of include/fsea.h");

// a tile's partial as the fold reads it: the six sums, the largest P and the job's index of the first pair that has it
struct Partial {
    double sum[6];
    double peak;
    unsigned long long peak_index;
};
static_assert(sizeof(Partial) == 64, "eight lanes store a partial, 8 bytes each");

// one accumulator of a fold: s_re, s_im, p, q, r_re, r_im in sum[]; (peak, at) starts at (+0.0, 0), which is what a job or a
// tile of nothing but zeros has and what loses against any P above zero
struct Lane {
    double sum[6];
    double peak;
    unsigned long long at;
};

__device__ __forceinline__ Lane lane_zero() { return Lane{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0, 0ull}; }

// the larger peak, the smaller index among equal ones
__device__ __forceinline__ void keep_peak(Lane &a, double peak, unsigned long long at) {
    if (peak > a.peak || (peak == a.peak && at < a.at)) {
        a.peak = peak;
        a.at = at;
    }
}

// The terms of one pair z (tile index t) and of its partner w.  WHOLE: both are there.  Otherwise `valid` says whether the
// tile has a pair t at all and `lagged` whether it has a partner; what is absent is +0.0, which leaves an accumulator as it
// is (none is ever -0.0), and the loads behind z and w were of some other pair of the job.
template <bool WHOLE>
__device__ __forceinline__ void add_pair(Lane &a, float2 z, float2 w, bool valid, bool lagged, double off_re, double off_im, unsigned t) {
    const double x = (double)z.x - off_re, y = (double)z.y - off_im;
    const double u = (double)w.x - off_re, v = (double)w.y - off_im;
    const double p = x * x + y * y;
    const double q = p * p;
    const double r_re = x * u + y * v;
    const double r_im = y * u - x * v;
    a.sum[0] += WHOLE || valid ? x : 0.0;
    a.sum[1] += WHOLE || valid ? y : 0.0;
    a.sum[2] += WHOLE || valid ? p : 0.0;
    a.sum[3] += WHOLE || valid ? q : 0.0;
    a.sum[4] += WHOLE || lagged ? r_re : 0.0;
    a.sum[5] += WHOLE || lagged ? r_im : 0.0;
    if ((WHOLE || valid) && p > a.peak) {   // a lane's t only grows: the first pair that has the peak stays
        a.peak = p;
        a.at = t;
    }
}

// Lane tid's sixteen pairs of the tile that begins at pair i0 of the job whose pair 0 is at `job`: all thirty-two loads, then
// the arithmetic.  WHOLE: n_tile == MS_TILE and i0 >= lag, every pair and every partner is there, and a load is a uniform
// base and the lane's offset.  Otherwise a pair past the tile's end is loaded as the tile's last and a partner in front of
// the job as the pair itself: every load stays inside the job, and add_pair leaves those terms out.
template <bool WHOLE>
__device__ __forceinline__ void tile_terms(Lane &a, const float2 *__restrict__ job, unsigned i0, unsigned n_tile, unsigned lag,
                                           double off_re, double off_im, unsigned tid) {
    float2 zs[MS_STEPS], ws[MS_STEPS];
    const float2 *__restrict__ z = job + i0;
    const float2 *__restrict__ back = job + (WHOLE ? i0 - lag : 0u);
#pragma unroll
    for (int s = 0; s < MS_STEPS; ++s) {
        const unsigned t = tid + MS_WG * s;
        if (WHOLE) {
            zs[s] = z[t];
            ws[s] = back[t];
        } else {
            const unsigned i = i0 + (t < n_tile ? t : n_tile - 1u);
            zs[s] = job[i];
            ws[s] = job[i >= lag ? i - lag : i];
        }
    }
#pragma unroll
    for (int s = 0; s < MS_STEPS; ++s) {
        const unsigned t = tid + MS_WG * s;
        __builtin_amdgcn_sched_barrier(0);   // a pair's terms after the previous pair's: nothing of the sixteen is worked ahead
        add_pair<WHOLE>(a, zs[s], ws[s], t < n_tile, t < n_tile && i0 + t >= lag, off_re, off_im, t);
    }
}

// the xor stages k = 1 .. 32 of a fold over a wave's 64 accumulators: every lane ends with acc[0]'s value
__device__ __forceinline__ void wave_fold(Lane &a) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
        for (int c = 0; c < 6; ++c) a.sum[c] = a.sum[c] + __shfl_xor(a.sum[c], k, 64);
        const double peak = __shfl_xor(a.peak, k, 64);
        const unsigned long long at = __shfl_xor(a.at, k, 64);
        keep_peak(a, peak, at);
    }
}

}  // namespace

// grid: the tiles of all jobs; tile0[k] is job k's first tile, a job's tiles follow one another
extern "C" __global__ __launch_bounds__(MS_WG, 4) void fsea_measure_tiles(const float2 *__restrict__ pairs,
                                                                      const fsea_measure_job *__restrict__ jobs,
                                                                      const uint32_t *__restrict__ tile0, int n_jobs, int steps,
                                                                      double off_re, double off_im, int lag,
                                                                      Partial *__restrict__ partials) {
    __shared__ Lane part[MS_WG / 64];
    const unsigned tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;

    const int lo = fsea_detail::job_of_tile(tile0, n_jobs, steps, tile);
    const unsigned long long first = jobs[lo].first_pair, n = jobs[lo].n_pairs;
    const unsigned i0 = (tile - tile0[lo]) * (unsigned)MS_TILE;    // the tile's first pair, counted from the job's: below 2^24
    const unsigned left = (unsigned)n - i0;                         // pairs from there on: at least 1
    const unsigned n_tile = left < (unsigned)MS_TILE ? left : (unsigned)MS_TILE;

    Lane a = lane_zero();
    if (n_tile == (unsigned)MS_TILE && i0 >= (unsigned)lag) tile_terms<true>(a, pairs + first, i0, n_tile, (unsigned)lag, off_re, off_im, tid);
    else tile_terms<false>(a, pairs + first, i0, n_tile, (unsigned)lag, off_re, off_im, tid);
    wave_fold(a);
    if ((tid & 63) == 0) part[tid >> 6] = a;
    __syncthreads();
    // stages k = 64 and 128: acc[0] = (w0 + w1) + (w2 + w3); lanes 0 .. 5 a sum each, lanes 6 and 7 the peak and its index
    if (tid < 8) {
        unsigned long long bits;
        if (tid < 6) {
            bits = (unsigned long long)__double_as_longlong((part[0].sum[tid] + part[1].sum[tid]) + (part[2].sum[tid] + part[3].sum[tid]));
        } else {
            Lane best = part[0];
#pragma unroll
            for (int w = 1; w < MS_WG / 64; ++w) keep_peak(best, part[w].peak, part[w].at);
            bits = tid == 6 ? (unsigned long long)__double_as_longlong(best.peak) : (unsigned long long)i0 + best.at;
        }
        reinterpret_cast<unsigned long long *>(partials + tile)[tid] = bits;
    }
}

// grid: one wave per job
extern "C" __global__ __launch_bounds__(64) void fsea_measure_fold(const fsea_measure_job *__restrict__ jobs,
                                                                  const uint32_t *__restrict__ tile0,
                                                                  const Partial *__restrict__ partials, int lag,
                                                                  fsea_measure_sums *__restrict__ sums) {
    const int lane = threadIdx.x;
    const uint32_t k = blockIdx.x;
    const unsigned long long n = jobs[k].n_pairs;
    const int tiles = (int)((n + MS_TILE - 1) / MS_TILE);
    const Partial *__restrict__ mine = partials + tile0[k];
    Lane a = lane_zero();
    for (int t = lane; t < tiles; t += 64) {
        const Partial p = mine[t];
#pragma unroll
        for (int c = 0; c < 6; ++c) a.sum[c] += p.sum[c];
        keep_peak(a, p.peak, p.peak_index);
    }
    wave_fold(a);
    if (lane == 0) {
        fsea_measure_sums r;
        r.s_re = a.sum[0];
        r.s_im = a.sum[1];
        r.p = a.sum[2];
        r.q = a.sum[3];
        r.r_re = a.sum[4];
        r.r_im = a.sum[5];
        r.peak = a.peak;
        r.peak_index = a.at;
        r.n_pairs = n;
        r.n_lagged = n > (unsigned long long)lag ? n - (unsigned long long)lag : 0;
        sums[k] = r;
    }
}

struct fsea_measure {
    int device = 0;
    fsea_detail::JobTable table;          // the jobs and their first-tile column; behind them in its scratch, the tile partials
    std::mutex mu;
    fsea_detail::HostStaging staging;     // the host form
};

namespace {

// Everything a run checks, in the header's order, reading nothing of the object.
int check_run(const fsea_measure *m, const void *pairs, size_t n_buffer_pairs, const fsea_measure_job *jobs, size_t n_jobs,
              double offset_re, double offset_im, int lag, const void *sums) {
    if (int rc = fsea_detail::check_jobs_head(m, "measure", n_jobs, jobs, pairs, sums)) return rc;
    if (n_jobs == 0) return FSEA_OK;
    if (lag < 1 || lag > FSEA_MEASURE_MAX_LAG) return fail(FSEA_EINVAL, "lag must be in [1, %d], got %d", FSEA_MEASURE_MAX_LAG, lag);
    if (int rc = fsea_detail::check_offset(offset_re, offset_im)) return rc;
    uint64_t total = 0;
    for (size_t i = 0; i < n_jobs; ++i) {
        const fsea_measure_job &j = jobs[i];
        if (int rc = fsea_detail::check_job_span(i, j.first_pair, j.n_pairs, n_buffer_pairs, FSEA_MEASURE_MAX_PAIRS, "pairs", "buffer")) return rc;
        total += j.n_pairs;
    }
    return fsea_detail::check_jobs_total(total, "pairs");
}

// One call on device buffers, asynchronous on `s`: the table built in mapped host memory, its upload, the tiles, the fold.
// The caller holds m->mu and is on m's device; the arguments are checked and n_jobs is at least 1.
int queue_call(fsea_measure *m, const void *d_pairs, const fsea_measure_job *jobs, size_t n_jobs, double offset_re, double offset_im,
               int lag, fsea_measure_sums *d_sums, hipStream_t s) {
    fsea_detail::JobTable::Built<fsea_measure_job> t;
    const int rc = m->table.build<fsea_measure_job>(n_jobs, MS_TILE, sizeof(Partial), s, [&](size_t i, fsea_measure_job &rec, uint32_t) {
        rec = jobs[i];
        return jobs[i].n_pairs;
    }, &t);
    if (rc) return rc;
    Partial *d_partials = reinterpret_cast<Partial *>(t.behind);
    if (t.tiles) {
        hipLaunchKernelGGL(fsea_measure_tiles, dim3((unsigned)t.tiles), dim3(MS_WG), 0, s, static_cast<const float2 *>(d_pairs), t.recs,
                           t.tile0, (int)n_jobs, fsea_detail::job_steps(n_jobs), offset_re, offset_im, lag, d_partials);
        FSEA_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(fsea_measure_fold, dim3((unsigned)n_jobs), dim3(64), 0, s, t.recs, t.tile0, static_cast<const Partial *>(d_partials),
                       lag, d_sums);
    FSEA_HIP(hipGetLastError());
    return m->table.release(s);
}

}  // namespace

extern "C" {

int fsea_measure_create(fsea_measure **out, int device) {
    if (!out) return fail(FSEA_EINVAL, "measure out-pointer is NULL");
    *out = nullptr;
    return fsea_detail::create_object(out, device, "fsea_measure_create",
                                      [&](fsea_measure *m) -> hipError_t { return m->table.create(m->staging.stream); });
}

int fsea_measure_destroy(fsea_measure *m) { return fsea_detail::destroy_object(m); }

int fsea_measure_run_device(fsea_measure *m, const void *d_pairs, size_t n_buffer_pairs, const fsea_measure_job *jobs, size_t n_jobs,
                            double offset_re, double offset_im, int lag, fsea_measure_sums *d_sums, void *stream) {
    const int rc = check_run(m, d_pairs, n_buffer_pairs, jobs, n_jobs, offset_re, offset_im, lag, d_sums);
    if (rc || n_jobs == 0) return rc;
    return fsea_detail::run_device_pairs(m, d_pairs, d_sums, "d_sums", 16, stream, [&](hipStream_t s) {
        return queue_call(m, d_pairs, jobs, n_jobs, offset_re, offset_im, lag, d_sums, s);
    });
}

int fsea_measure_run_host(fsea_measure *m, const float *pairs, size_t n_buffer_pairs, const fsea_measure_job *jobs, size_t n_jobs,
                          double offset_re, double offset_im, int lag, fsea_measure_sums *sums) {
    const int rc = check_run(m, pairs, n_buffer_pairs, jobs, n_jobs, offset_re, offset_im, lag, sums);
    if (rc || n_jobs == 0) return rc;
    const size_t end = fsea_detail::staged_pairs(jobs, n_jobs, [](const fsea_measure_job &j) { return j.n_pairs != 0; });
    std::lock_guard<std::mutex> lock(m->mu);
    FSEA_ON_DEVICE(m->device);
    return m->staging.run(
        end * sizeof(float2), n_jobs * sizeof(fsea_measure_sums), sums, [&](void *h_in) { std::memcpy(h_in, pairs, end * sizeof(float2)); },
        [&](void *d_in, void *d_out, hipStream_t s) {
            return queue_call(m, d_in, jobs, n_jobs, offset_re, offset_im, lag, static_cast<fsea_measure_sums *>(d_out), s);
        });
}

int fsea_measure_jobs(const fsea_extract_job *ejobs, size_t n_jobs, int decimation, size_t skip_pairs, fsea_measure_job *jobs) {
    return fsea_detail::jobs_of_extract(ejobs, n_jobs, decimation, skip_pairs, FSEA_MEASURE_MAX_PAIRS, jobs, [](fsea_measure_job &) {});
}

// Host arithmetic; no device is touched.  Each line is the header's formula; 0 / 0 gives the NaN of an empty or silent job.
int fsea_measure_finish(const fsea_measure_sums *sums, int lag, fsea_measure_result *result) {
    if (!sums || !result) return fail(FSEA_EINVAL, "NULL buffer");
    if (lag < 1 || lag > FSEA_MEASURE_MAX_LAG) return fail(FSEA_EINVAL, "lag must be in [1, %d], got %d", FSEA_MEASURE_MAX_LAG, lag);
    const double n = (double)sums->n_pairs, m = (double)sums->n_lagged, nan = std::nan("");
    const double turn = 2.0 * M_PI * (double)lag;
    fsea_measure_result r;
    r.mean_power = sums->p / n;
    r.power_db = 10.0 * std::log10(r.mean_power);
    r.dc_re = sums->s_re / n;
    r.dc_im = sums->s_im / n;
    r.kurtosis = n * sums->q / (sums->p * sums->p);
    r.crest = sums->peak * n / sums->p;
    r.peak_index = sums->peak_index;
    r.n_pairs = sums->n_pairs;
    r.freq_cycles = r.coherence = r.width_cycles = nan;
    if (sums->n_lagged) {
        const double ratio = std::hypot(sums->r_re, sums->r_im) * n / (sums->p * m);
        r.freq_cycles = std::atan2(sums->r_im, sums->r_re) / turn;
        r.coherence = ratio > 1.0 ? 1.0 : ratio;   // a NaN stays one
        r.width_cycles = std::sqrt(-2.0 * std::log(r.coherence) + 0.0) / turn;
    }
    *result = r;
    return FSEA_OK;
}

}  // extern "C"
