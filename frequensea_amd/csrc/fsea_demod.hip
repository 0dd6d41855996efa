// fsea_demod.hip -- the reference's audio chain (src/nrf.c:778-1094: nrf_downsampler, nrf_raw_demodulator,
// nrf_fm_demodulator, nrf_decoder) as a streaming, multi-channel decoder (include/fsea.h: fsea_demod_*).  Every channel
// reads the same input stream with its own frequency offset, phase and state.  Arithmetic in f64, like the reference.
//
// Per call on n input samples, channel ch:
//   x[k]      = (c + i s) e^{i theta k} (u8[2k] / 128 - 0.995, u8[2k+1] / 128 - 0.995),   theta = 2 pi offset / in_rate
//   stage 1   y1[j] = sum_{m < L1} c1[m] x_ext[idx1[j] + m],  x_ext = tail1 ++ x          (I only for RAW: the audio)
//   stage 2   the reference's discriminator on (y1[j - 1], y1[j]), y1[-1] = l carried from the last call
//   stage 3   y3[j] = sum_{m < L3} c3[m] d_ext[idx3[j] + m],  d_ext = tail3 ++ discriminator outputs
//   stage 4   v = v + alpha (y3[j] - v), v carried
// idx[j] is the reference's accumulated floor(t), t += rate_mul from 0 on every call; the tables are built on the host.
//
// Kernels ("The audio decoder"):
//   fsea_demod_stage1_*  grid (tiles of stage-1 outputs, channels), 256 lanes.  A tile of T outputs stages the x_ext span it
//                        reads (at most DM_SPAN samples) in LDS, converted and rotated once; each lane computes one output.
//                        The phase of each group of 8 samples is seeded from the exactly reduced cycle count
//                        (offset k mod in_rate) / in_rate by sincospi and advanced by a 7-step recurrence.  Workgroup
//                        (0, ch) writes the next tail.
//   fsea_demod_fm        grid (tiles of audio outputs, channels): stages the discriminator outputs of its span in LDS,
//                        then one lane per audio output; workgroup (0, ch) writes the next l and stage-3 tail.
//   fsea_demod_deemph    one workgroup per channel: the first-order recurrence as chunks of consecutive samples per lane,
//                        chained by a scan of the chunks' affine maps, then re-run from each chunk's start value.
// Every piece of state (tails, l, the de-emphasis value) lives in two device buffers used in turn, so no launch
// overwrites a value a workgroup of the same call still reads.  The channel index selects rows and parameters only.
#include "fsea_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

using fsea_detail::DeviceArray;
using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int DM_WG = 256;           // lanes per workgroup
constexpr int DM_SPAN = 4096;        // x_ext samples one tile stages at most
constexpr int DM_TAIL = 64;          // tail row pitch (>= L - 1 of every stage)
constexpr int DM_RING = 4;           // channel-parameter slots in flight
constexpr int DM_CACHE = 8;          // index tables kept per object
constexpr int L_RAW = 41, L_FM1 = 51, L_FM3 = 41;
constexpr int FM_INTER_RATE = 336000, FM_MAX_F = 75000;
constexpr double TAU = M_PI * 2;

enum { DM_IN_U8 = 0, DM_IN_F64 = 1 };

struct ChanParam {
    long long off;   // offset mod in_rate, in [0, in_rate)
    double c, s;     // phase of sample 0 of the call
};

// (c, s) of input sample `g` (a multiple of 8): the channel's start phase times e^{2 pi i (off g mod rate) / rate}
__device__ __forceinline__ void seed_phase(long long g, const ChanParam &p, int rate, double &c, double &s) {
    const unsigned long long m = ((unsigned long long)p.off * (unsigned long long)(g % rate)) % (unsigned long long)rate;
    double sp, cp;
    sincospi(2.0 * (double)m / (double)rate, &sp, &cp);
    c = p.c * cp - p.s * sp;
    s = p.c * sp + p.s * cp;
}

template <int KIND>
__device__ __forceinline__ void load_raw(const void *in0, const void *in1, long long k, uint32_t flip, double &vi,
                                         double &vq) {
    if (KIND == DM_IN_U8) {
        const uint32_t b = ((uint32_t)(static_cast<const uint16_t *>(in0))[k] ^ flip) & 0xffffu;
        vi = (double)(b & 0xffu) / 128.0 - 0.995;
        vq = (double)(b >> 8) / 128.0 - 0.995;
    } else {
        vi = static_cast<const double *>(in0)[k];
        vq = static_cast<const double *>(in1)[k];
    }
}

// the 8 rotated samples g .. g + 7 (g >= 0, a multiple of 8); samples at or past n are zero
template <int KIND>
__device__ __forceinline__ void rotated_group(const void *in0, const void *in1, long long n, uint32_t flip, int rate,
                                              const ChanParam &p, double dc, double ds, long long g, double vi[8],
                                              double vq[8]) {
    double c, s;
    seed_phase(g, p, rate, c, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double ri = 0.0, rq = 0.0;
        if (g + j < n) load_raw<KIND>(in0, in1, g + j, flip, ri, rq);
        vi[j] = ri * c - rq * s;
        vq[j] = ri * s + rq * c;
        const double ns = c * ds + s * dc;
        const double nc = c * dc - s * ds;
        s = ns;
        c = nc;
    }
}

template <int KIND, bool IQ>
__device__ __forceinline__ void stage1_body(const void *__restrict__ in0, const void *__restrict__ in1, long long n,
                                            uint32_t flip, int rate, const ChanParam *__restrict__ par,
                                            const double2 *__restrict__ tail_in, double2 *__restrict__ tail_out, int L,
                                            const double *__restrict__ taps, const int *__restrict__ idx, int n1, int T,
                                            double *__restrict__ out, long long ld) {
    __shared__ double lds_i[DM_SPAN];
    __shared__ double lds_q[IQ ? DM_SPAN : 1];
    const int tid = threadIdx.x;
    const int ch = blockIdx.y;
    const ChanParam p = par[ch];
    double ds, dc;
    sincospi(2.0 * (double)p.off / (double)rate, &ds, &dc);
    const double2 *tin = tail_in + (size_t)ch * DM_TAIL;
    const long long j0 = (long long)blockIdx.x * T;

    if (j0 < n1) {
        const int jl = (int)(j0 + T <= n1 ? j0 + T - 1 : n1 - 1);
        const long long p0 = idx[j0];                         // first x_ext position of the tile
        const int span = idx[jl] - (int)p0 + L;               // <= DM_SPAN (the host picked T so)
        const long long s_first = p0 - (L - 1);               // its input sample (negative: the tail)
        const long long s_al = s_first >= 0 ? (s_first & ~7LL) : -((-s_first + 7) & ~7LL);
        const int groups = (int)((s_first - s_al + span + 7) >> 3);
        for (int gi = tid; gi < groups; gi += DM_WG) {
            const long long g = s_al + 8LL * gi;
            double vi[8], vq[8];
            if (g >= 0) {
                rotated_group<KIND>(in0, in1, n, flip, rate, p, dc, ds, g, vi, vq);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long long t = g + j + (L - 1);
                    const double2 v = t >= 0 ? tin[t] : double2{0.0, 0.0};
                    vi[j] = v.x;
                    vq[j] = v.y;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long i = g + j - s_first;
                if (i >= 0 && i < span) {
                    lds_i[i] = vi[j];
                    if (IQ) lds_q[i] = vq[j];
                }
            }
        }
        __syncthreads();
        const long long j = j0 + tid;
        if (tid < T && j < n1) {
            const int b = idx[j] - (int)p0;
            double si = 0.0, sq = 0.0;
            for (int m = 0; m < L; ++m) {
                const double c = taps[m];
                si += c * lds_i[b + m];
                if (IQ) sq += c * lds_q[b + m];
            }
            if (IQ) {
                reinterpret_cast<double2 *>(out)[(size_t)ch * ld + j] = double2{si, sq};
            } else {
                out[(size_t)ch * ld + j] = si;
            }
        }
    }

    // the next call's tail: x_ext[n + m], m < L - 1 (from the old tail while n + m < L - 1)
    if (blockIdx.x == 0) {
        for (int m = tid; m < L - 1; m += DM_WG) {
            const long long e = n + m;
            double2 v;
            if (e < L - 1) {
                v = tin[e];
            } else {
                const long long k = e - (L - 1);
                double vi[8], vq[8];
                rotated_group<KIND>(in0, in1, n, flip, rate, p, dc, ds, k & ~7LL, vi, vq);
                v = double2{vi[k & 7], vq[k & 7]};
            }
            tail_out[(size_t)ch * DM_TAIL + m] = v;
        }
    }
}

// the reference's discriminator (src/nrf.c:969-993) on the previous and the current stage-1 output, operation for operation
__device__ __forceinline__ double discriminate(double2 l, double2 y, double ampl_conv) {
#pragma clang fp contract(off)
    double real = l.x * y.x + l.y * y.y;
    double imag = l.x * y.y - y.x * l.y;
    double sgn = 1;
    if (imag < 0) {
        sgn *= -1;
        imag *= -1;
    }
    double ang = 0;
    double div;
    if (real == imag) {
        div = 1;
    } else if (real > imag) {
        div = imag / real;
    } else {
        ang = -M_PI / 2;
        div = real / imag;
        sgn *= -1;
    }
    return sgn * (ang + div / (0.98419158358617365 + div * (0.093485702629671305 + div * 0.19556307900617517))) *
           ampl_conv;
}

// discriminator output i of this call: y1[i] against y1[i - 1], or against the carried l for i = 0
__device__ __forceinline__ double disc_at(const double2 *y1, long long i, double2 l, double ampl_conv) {
    double2 prev = l;
    if (i > 0) prev = y1[i - 1];
    return discriminate(prev, y1[i], ampl_conv);
}

}  // namespace

extern "C" __global__ __launch_bounds__(DM_WG) void fsea_demod_stage1_u8(
    const void *__restrict__ in0, const void *__restrict__ in1, long long n, uint32_t flip, int rate,
    const ChanParam *__restrict__ par, const double2 *__restrict__ tail_in, double2 *__restrict__ tail_out, int L,
    const double *__restrict__ taps, const int *__restrict__ idx, int n1, int T, double *__restrict__ out, long long ld) {
    stage1_body<DM_IN_U8, true>(in0, in1, n, flip, rate, par, tail_in, tail_out, L, taps, idx, n1, T, out, ld);
}

extern "C" __global__ __launch_bounds__(DM_WG) void fsea_demod_stage1_f64(
    const void *__restrict__ in0, const void *__restrict__ in1, long long n, uint32_t flip, int rate,
    const ChanParam *__restrict__ par, const double2 *__restrict__ tail_in, double2 *__restrict__ tail_out, int L,
    const double *__restrict__ taps, const int *__restrict__ idx, int n1, int T, double *__restrict__ out, long long ld) {
    stage1_body<DM_IN_F64, true>(in0, in1, n, flip, rate, par, tail_in, tail_out, L, taps, idx, n1, T, out, ld);
}

extern "C" __global__ __launch_bounds__(DM_WG) void fsea_demod_stage1_u8_i(
    const void *__restrict__ in0, const void *__restrict__ in1, long long n, uint32_t flip, int rate,
    const ChanParam *__restrict__ par, const double2 *__restrict__ tail_in, double2 *__restrict__ tail_out, int L,
    const double *__restrict__ taps, const int *__restrict__ idx, int n1, int T, double *__restrict__ out, long long ld) {
    stage1_body<DM_IN_U8, false>(in0, in1, n, flip, rate, par, tail_in, tail_out, L, taps, idx, n1, T, out, ld);
}

extern "C" __global__ __launch_bounds__(DM_WG) void fsea_demod_stage1_f64_i(
    const void *__restrict__ in0, const void *__restrict__ in1, long long n, uint32_t flip, int rate,
    const ChanParam *__restrict__ par, const double2 *__restrict__ tail_in, double2 *__restrict__ tail_out, int L,
    const double *__restrict__ taps, const int *__restrict__ idx, int n1, int T, double *__restrict__ out, long long ld) {
    stage1_body<DM_IN_F64, false>(in0, in1, n, flip, rate, par, tail_in, tail_out, L, taps, idx, n1, T, out, ld);
}

// stages 2 and 3: y1 rows of pitch ld1 (n1 valid), audio rows of pitch ld2 (n2 valid, before de-emphasis)
extern "C" __global__ __launch_bounds__(DM_WG) void fsea_demod_fm(
    const double2 *__restrict__ y1all, long long n1, long long ld1, const double2 *__restrict__ l_in,
    double2 *__restrict__ l_out, const double *__restrict__ tail_in, double *__restrict__ tail_out, int L,
    const double *__restrict__ taps, const int *__restrict__ idx, int n2, int T, double ampl_conv,
    double *__restrict__ audio, long long ld2) {
    __shared__ double lds[DM_SPAN];
    const int tid = threadIdx.x;
    const int ch = blockIdx.y;
    const double2 *y1 = y1all + (size_t)ch * ld1;
    const double2 l = l_in[ch];
    const double *tin = tail_in + (size_t)ch * DM_TAIL;
    const long long j0 = (long long)blockIdx.x * T;

    if (j0 < n2) {
        const int jl = (int)(j0 + T <= n2 ? j0 + T - 1 : n2 - 1);
        const int p0 = idx[j0];
        const int span = idx[jl] - p0 + L;
        for (int i = tid; i < span; i += DM_WG) {
            const long long e = (long long)p0 + i;     // d_ext position
            lds[i] = e < L - 1 ? tin[e] : disc_at(y1, e - (L - 1), l, ampl_conv);
        }
        __syncthreads();
        const long long j = j0 + tid;
        if (tid < T && j < n2) {
            const int b = idx[j] - p0;
            double acc = 0.0;
            for (int m = 0; m < L; ++m) acc += taps[m] * lds[b + m];
            audio[(size_t)ch * ld2 + j] = acc;
        }
    }

    if (blockIdx.x == 0) {
        for (int m = tid; m < L - 1; m += DM_WG) {
            const long long e = n1 + m;
            tail_out[(size_t)ch * DM_TAIL + m] = e < L - 1 ? tin[e] : disc_at(y1, e - (L - 1), l, ampl_conv);
        }
        if (tid == 0) {
            double2 last = l;
            if (n1 > 0) last = y1[n1 - 1];
            l_out[ch] = last;
        }
    }
}

// stage 4, in place on the audio rows
extern "C" __global__ __launch_bounds__(DM_WG) void fsea_demod_deemph(double *__restrict__ audio, int n2, long long ld,
                                                                       double alpha, const double *__restrict__ v_in,
                                                                       double *__restrict__ v_out) {
#pragma clang fp contract(off)
    __shared__ double sa[DM_WG], sb[DM_WG];
    const int tid = threadIdx.x;
    const int ch = blockIdx.x;
    double *row = audio + (size_t)ch * ld;
    const double v0 = v_in[ch];
    const int chunk = (n2 + DM_WG - 1) / DM_WG;
    const int lo = min(n2, tid * chunk), hi = min(n2, lo + chunk);

    // this chunk's map v -> a v + b: b from the reference's loop started at 0, a = (1 - alpha)^len
    double a = 1.0, b = 0.0;
    for (int i = lo; i < hi; ++i) {
        b = b + alpha * (row[i] - b);
        a = a * (1.0 - alpha);
    }
    sa[tid] = a;
    sb[tid] = b;
    __syncthreads();
    // inclusive scan of the maps (Hillis-Steele): entry t becomes chunks 0..t composed
    for (int d = 1; d < DM_WG; d <<= 1) {
        double pa = 1.0, pb = 0.0;
        if (tid >= d) {
            pa = sa[tid - d];
            pb = sb[tid - d];
        }
        __syncthreads();
        if (tid >= d) {
            const double ca = sa[tid], cb = sb[tid];
            sa[tid] = ca * pa;
            sb[tid] = ca * pb + cb;
        }
        __syncthreads();
    }
    double v = tid == 0 ? v0 : sa[tid - 1] * v0 + sb[tid - 1];
    for (int i = lo; i < hi; ++i) {
        v = v + alpha * (row[i] - v);
        row[i] = v;
    }
    if (n2 == 0) {
        if (tid == 0) v_out[ch] = v0;
    } else if (lo < hi && hi == n2) {
        v_out[ch] = v;
    }
}

namespace {

struct Table {
    size_t n = 0;                 // input samples of the call
    int n1 = 0, n2 = 0, T1 = 0, T3 = 0;
    DeviceArray<int> d_idx1, d_idx3;
    unsigned long long use = 0;
};

}  // namespace

struct fsea_demod {
    int type = 0, in_rate = 0, out_rate = 0, K = 0, device = 0;
    int L1 = 0, L3 = 0;
    double r1 = 0.0, r3 = 0.0, ampl_conv = 0.0, alpha = 0.0;
    DeviceArray<double> d_taps1, d_taps3;       // DM_TAIL taps each, zeros past L
    DeviceArray<double2> d_tail1[2];            // K rows of DM_TAIL rotated samples
    DeviceArray<double> d_tail3[2];             // K rows of DM_TAIL discriminator outputs
    DeviceArray<double2> d_l[2];                // K carried stage-1 outputs
    DeviceArray<double> d_v[2];                 // K de-emphasis values
    int cur = 0;
    struct Chan {
        int offset = 0;
        double c = 1.0, s = 0.0;
    };
    std::vector<Chan> chan;
    struct Slot {                               // the K channel parameters of one call, on their way to the device
        DeviceArray<ChanParam> d_par;
        fsea_detail::PinnedArray<ChanParam> h_par;
        fsea_detail::Event ev;                  // recorded behind the call that read d_par
        bool used = false;
    } slots[DM_RING];
    int ring = 0;
    std::vector<Table> tables;
    unsigned long long use_seq = 0;
    std::mutex mu;
    fsea_detail::DeviceBuffer y1;               // stage 1's outputs of a WBFM call
    fsea_detail::HostStaging staging;           // the host-buffer forms
};

namespace {

// the reference's out_length = floor(length / rate_mul)
long long stage_length(long long n, double r) { return (long long)floor((double)n / r); }

// outputs per call of each stage; false when a stage would exceed FSEA_DEMOD_MAX_SAMPLES outputs
bool lengths(const fsea_demod *d, size_t n, long long *n1, long long *n2) {
    *n1 = stage_length((long long)n, d->r1);
    *n2 = d->type == FSEA_DEMOD_WBFM ? stage_length(*n1, d->r3) : *n1;
    return *n1 <= FSEA_DEMOD_MAX_SAMPLES && *n2 <= FSEA_DEMOD_MAX_SAMPLES;
}

// the reference's accumulated floor(t) for `count` outputs, and the largest tile T <= DM_WG whose spans fit DM_SPAN
void index_table(int count, double r, int L, std::vector<int> &idx, int *T) {
    idx.resize(count);
    double t = 0;
    for (int j = 0; j < count; ++j) {
        idx[j] = (int)floor(t);
        t += r;
    }
    int tt = DM_WG;
    for (;;) {
        bool ok = true;
        for (int j0 = 0; j0 < count && ok; j0 += tt) {
            const int jl = j0 + tt <= count ? j0 + tt - 1 : count - 1;
            ok = idx[jl] - idx[j0] + L <= DM_SPAN;
        }
        if (ok || tt == 1) break;
        tt = tt > 16 ? tt - tt / 8 : tt - 1;
    }
    *T = tt;
}

// the cached tables for calls of n samples; the caller holds d->mu and is on d's device
int tables_for(fsea_demod *d, size_t n, const Table **out) {
    for (Table &t : d->tables) {
        if (t.n == n) {
            t.use = ++d->use_seq;
            *out = &t;
            return FSEA_OK;
        }
    }
    long long n1, n2;
    if (!lengths(d, n, &n1, &n2)) return fail(FSEA_EINVAL, "n_samples %zu gives more than %d outputs", n, FSEA_DEMOD_MAX_SAMPLES);
    Table t;
    t.n = n;
    t.n1 = (int)n1;
    t.n2 = (int)n2;
    std::vector<int> idx1, idx3;
    index_table(t.n1, d->r1, d->L1, idx1, &t.T1);
    if (t.n1 > 0 && idx1.back() > (long long)n - 1) return fail(FSEA_EINVAL, "rate %g does not fit n_samples %zu", d->r1, n);
    if (d->type == FSEA_DEMOD_WBFM) {
        index_table(t.n2, d->r3, d->L3, idx3, &t.T3);
        if (t.n2 > 0 && idx3.back() > n1 - 1) return fail(FSEA_EINVAL, "rate %g does not fit %lld samples", d->r3, n1);
    }
    FSEA_HIP(t.d_idx1.upload(idx1.data(), idx1.size()));
    FSEA_HIP(t.d_idx3.upload(idx3.data(), idx3.size()));
    if ((int)d->tables.size() >= DM_CACHE) {
        size_t lru = 0;
        for (size_t i = 1; i < d->tables.size(); ++i)
            if (d->tables[i].use < d->tables[lru].use) lru = i;
        FSEA_HIP(hipDeviceSynchronize());   // launches on any stream may still read it
        d->tables.erase(d->tables.begin() + (long)lru);   // the tables behind it move down; the evicted arrays are freed
    }
    t.use = ++d->use_seq;
    d->tables.push_back(std::move(t));
    *out = &d->tables.back();
    return FSEA_OK;
}

long long offset_mod(int offset, int rate) {
    long long m = (long long)offset % rate;
    return m < 0 ? m + rate : m;
}

// one call: parameters, the stage kernels, the phase advance; the caller holds d->mu and is on d's device
int demod_launch(fsea_demod *d, int kind, const void *in0, const void *in1, size_t n, int flip, double *d_audio,
                 hipStream_t s) {
    const Table *t = nullptr;
    int rc = tables_for(d, n, &t);
    if (rc) return rc;
    if (d->type == FSEA_DEMOD_WBFM) {
        const size_t y1_bytes = (size_t)d->K * (size_t)(t->n1 > 0 ? t->n1 : 1) * sizeof(double2);
        if (d->y1.ptr && d->y1.cap < y1_bytes) {
            FSEA_HIP(hipDeviceSynchronize());   // a launch on another stream may still use the old buffer
        }
        rc = d->y1.grow(y1_bytes);
        if (rc) return rc;
    }
    fsea_demod::Slot &slot = d->slots[d->ring];
    if (slot.used) FSEA_HIP(hipEventSynchronize(slot.ev));   // the slot's last copy has been read
    for (int ch = 0; ch < d->K; ++ch) {
        slot.h_par.ptr[ch] = ChanParam{offset_mod(d->chan[ch].offset, d->in_rate), d->chan[ch].c, d->chan[ch].s};
    }
    FSEA_HIP(hipMemcpyAsync(slot.d_par.ptr, slot.h_par.ptr, (size_t)d->K * sizeof(ChanParam), hipMemcpyHostToDevice, s));

    const int cur = d->cur, nxt = d->cur ^ 1;
    const uint32_t fm = (kind == DM_IN_U8 && flip) ? 0x8080u : 0u;
    const long long nn = (long long)n;
    const unsigned g1 = (unsigned)(t->n1 > 0 ? (t->n1 + t->T1 - 1) / t->T1 : 1);
    const bool fm_chain = d->type == FSEA_DEMOD_WBFM;
    double *out1 = fm_chain ? static_cast<double *>(d->y1.ptr) : d_audio;
    const long long ld1 = fm_chain ? (t->n1 > 0 ? t->n1 : 1) : t->n1;
    auto k1 = kind == DM_IN_U8 ? (fm_chain ? fsea_demod_stage1_u8 : fsea_demod_stage1_u8_i)
                               : (fm_chain ? fsea_demod_stage1_f64 : fsea_demod_stage1_f64_i);
    hipLaunchKernelGGL(k1, dim3(g1, d->K), dim3(DM_WG), 0, s, in0, in1, nn, fm, d->in_rate, slot.d_par.ptr,
                       d->d_tail1[cur].ptr, d->d_tail1[nxt].ptr, d->L1, d->d_taps1.ptr, t->d_idx1.ptr, t->n1, t->T1, out1, ld1);
    FSEA_HIP(hipGetLastError());
    if (fm_chain) {
        const unsigned g3 = (unsigned)(t->n2 > 0 ? (t->n2 + t->T3 - 1) / t->T3 : 1);
        hipLaunchKernelGGL(fsea_demod_fm, dim3(g3, d->K), dim3(DM_WG), 0, s, static_cast<const double2 *>(d->y1.ptr),
                           (long long)t->n1, ld1, d->d_l[cur].ptr, d->d_l[nxt].ptr, d->d_tail3[cur].ptr, d->d_tail3[nxt].ptr,
                           d->L3, d->d_taps3.ptr, t->d_idx3.ptr, t->n2, t->T3, d->ampl_conv, d_audio, (long long)t->n2);
        FSEA_HIP(hipGetLastError());
        hipLaunchKernelGGL(fsea_demod_deemph, dim3(d->K), dim3(DM_WG), 0, s, d_audio, t->n2, (long long)t->n2, d->alpha,
                           d->d_v[cur].ptr, d->d_v[nxt].ptr);
        FSEA_HIP(hipGetLastError());
    }
    FSEA_HIP(hipEventRecord(slot.ev, s));
    slot.used = true;
    d->ring = (d->ring + 1) % DM_RING;
    d->cur = nxt;

    // the phase each channel starts its next call with: (c, s) e^{2 pi i (offset n mod in_rate) / in_rate}
    for (int ch = 0; ch < d->K; ++ch) {
        fsea_demod::Chan &c = d->chan[ch];
        const unsigned long long m = ((unsigned long long)offset_mod(c.offset, d->in_rate) *
                                      (unsigned long long)(n % (size_t)d->in_rate)) % (unsigned long long)d->in_rate;
        const double a = TAU * (double)m / (double)d->in_rate;
        const double ca = cos(a), sa = sin(a);
        const double nc = c.c * ca - c.s * sa, ns = c.c * sa + c.s * ca;
        c.c = nc;
        c.s = ns;
    }
    return FSEA_OK;
}

int check_call(const fsea_demod *d, size_t n) {
    if (!d) return fail(FSEA_EINVAL, "demod is NULL");
    if (n > FSEA_DEMOD_MAX_SAMPLES) return fail(FSEA_EINVAL, "n_samples %zu exceeds %d", n, FSEA_DEMOD_MAX_SAMPLES);
    long long n1, n2;
    if (!lengths(d, n, &n1, &n2)) return fail(FSEA_EINVAL, "n_samples %zu gives more than %d outputs", n, FSEA_DEMOD_MAX_SAMPLES);
    return FSEA_OK;
}

// the host-buffer forms: the launches through the object's staging (fsea_detail::HostStaging); f64 input is staged as
// the n I values, then the n Q values
int demod_host(fsea_demod *d, int kind, const void *in0, const void *in1, size_t n, int flip, double *audio) {
    int rc = check_call(d, n);
    if (rc) return rc;
    if (!in0 || (kind == DM_IN_F64 && !in1) || !audio) return fail(FSEA_EINVAL, "NULL buffer");
    if (n == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(d->mu);
    FSEA_ON_DEVICE(d->device);
    const size_t in_bytes = n * (kind == DM_IN_U8 ? 2 : 16);
    const size_t out_bytes = (size_t)d->K * fsea_demod_out_length(d, n) * sizeof(double);
    auto fill = [&](void *h_in) {
        if (kind == DM_IN_U8) {
            std::memcpy(h_in, in0, in_bytes);
        } else {
            std::memcpy(h_in, in0, n * 8);
            std::memcpy(static_cast<char *>(h_in) + n * 8, in1, n * 8);
        }
    };
    auto launch = [&](void *d_in, void *d_out, hipStream_t s) {
        const char *din = static_cast<const char *>(d_in);
        return demod_launch(d, kind, din, kind == DM_IN_U8 ? nullptr : din + n * 8, n, flip, static_cast<double *>(d_out), s);
    };
    return d->staging.run(in_bytes, out_bytes, audio, fill, launch);
}

int zero_state(fsea_demod *d) {
    for (int i = 0; i < 2; ++i) {
        FSEA_HIP(d->d_tail1[i].zero((size_t)d->K * DM_TAIL));
        FSEA_HIP(d->d_tail3[i].zero((size_t)d->K * DM_TAIL));
        FSEA_HIP(d->d_l[i].zero((size_t)d->K));
        FSEA_HIP(d->d_v[i].zero((size_t)d->K));
    }
    for (fsea_demod::Chan &c : d->chan) {
        c.c = 1.0;
        c.s = 0.0;
    }
    return FSEA_OK;
}

hipError_t upload_taps(DeviceArray<double> &dst, double rate, double cutoff, int L) {
    double taps[DM_TAIL] = {};
    if (fsea_fir_lowpass_taps(rate, cutoff, L, taps) != FSEA_OK) return hipErrorInvalidValue;
    return dst.upload(taps, DM_TAIL);
}

}  // namespace

extern "C" {

int fsea_demod_create(fsea_demod **out, int type, int in_rate, int out_rate, int n_channels, int device) {
    if (!out) return fail(FSEA_EINVAL, "demod out-pointer is NULL");
    *out = nullptr;
    if (type != FSEA_DEMOD_RAW && type != FSEA_DEMOD_WBFM) return fail(FSEA_EINVAL, "unknown demodulation type %d", type);
    if (in_rate <= 0 || out_rate <= 0) return fail(FSEA_EINVAL, "rates must be positive, got %d and %d", in_rate, out_rate);
    if (n_channels < 1 || n_channels > FSEA_DEMOD_MAX_CHANNELS) {
        return fail(FSEA_EINVAL, "n_channels must be in [1, %d], got %d", FSEA_DEMOD_MAX_CHANNELS, n_channels);
    }
    return fsea_detail::create_object(out, device, "fsea_demod_create", [&](fsea_demod *d) {
        d->type = type;
        d->in_rate = in_rate;
        d->out_rate = out_rate;
        d->K = n_channels;
        d->chan.resize(n_channels);
        // the reference's constructors: nrf_raw_demodulator_new, nrf_fm_demodulator_new (src/nrf.c:904-941)
        hipError_t e;
        if (type == FSEA_DEMOD_RAW) {
            d->L1 = L_RAW;
            d->r1 = in_rate / (double)out_rate;
            e = upload_taps(d->d_taps1, in_rate, out_rate / 2, L_RAW);
        } else {
            d->L1 = L_FM1;
            d->L3 = L_FM3;
            d->r1 = in_rate / (double)FM_INTER_RATE;
            d->r3 = FM_INTER_RATE / (double)out_rate;
            d->ampl_conv = out_rate / (TAU * FM_MAX_F);
            d->alpha = 1.0 / (1.0 + out_rate * 50.0 / 1e6);
            e = upload_taps(d->d_taps1, in_rate, (int)(FM_MAX_F * 0.8), L_FM1);
            if (e == hipSuccess) e = upload_taps(d->d_taps3, FM_INTER_RATE, 10000, L_FM3);
        }
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            e = d->d_tail1[i].alloc((size_t)n_channels * DM_TAIL);
            if (e == hipSuccess) e = d->d_tail3[i].alloc((size_t)n_channels * DM_TAIL);
            if (e == hipSuccess) e = d->d_l[i].alloc((size_t)n_channels);
            if (e == hipSuccess) e = d->d_v[i].alloc((size_t)n_channels);
        }
        for (int i = 0; i < DM_RING && e == hipSuccess; ++i) {
            e = d->slots[i].d_par.alloc((size_t)n_channels);
            if (e == hipSuccess) e = d->slots[i].h_par.alloc((size_t)n_channels);
            if (e == hipSuccess) e = d->slots[i].ev.create();
        }
        const int rc = fsea_detail::init_code("fsea_demod_create", e);
        return rc ? rc : zero_state(d);
    });
}

int fsea_demod_destroy(fsea_demod *d) { return fsea_detail::destroy_object(d); }

int fsea_demod_reset(fsea_demod *d) {
    return fsea_detail::reset_object(d, "demod is NULL", [&] { return zero_state(d); });
}

int fsea_demod_set_channel(fsea_demod *d, int ch, int freq_offset, double cosine, double sine) {
    if (!d) return fail(FSEA_EINVAL, "demod is NULL");
    if (ch < 0 || ch >= d->K) return fail(FSEA_EINVAL, "channel %d out of range [0,%d)", ch, d->K);
    if (!std::isfinite(cosine) || !std::isfinite(sine)) return fail(FSEA_EINVAL, "phase must be finite");
    std::lock_guard<std::mutex> lock(d->mu);
    d->chan[ch].offset = freq_offset;
    d->chan[ch].c = cosine;
    d->chan[ch].s = sine;
    return FSEA_OK;
}

int fsea_demod_get_channel(const fsea_demod *d, int ch, int *freq_offset, double *cosine, double *sine) {
    if (!d) return fail(FSEA_EINVAL, "demod is NULL");
    if (ch < 0 || ch >= d->K) return fail(FSEA_EINVAL, "channel %d out of range [0,%d)", ch, d->K);
    std::lock_guard<std::mutex> lock(const_cast<fsea_demod *>(d)->mu);
    if (freq_offset) *freq_offset = d->chan[ch].offset;
    if (cosine) *cosine = d->chan[ch].c;
    if (sine) *sine = d->chan[ch].s;
    return FSEA_OK;
}

size_t fsea_demod_out_length(const fsea_demod *d, size_t n_samples) {
    if (!d || n_samples > FSEA_DEMOD_MAX_SAMPLES) return 0;
    long long n1, n2;
    if (!lengths(d, n_samples, &n1, &n2)) return 0;
    return (size_t)n2;
}

int fsea_demod_u8_device(fsea_demod *d, const void *d_iq, size_t n_samples, int flip, double *d_audio, void *stream) {
    int rc = check_call(d, n_samples);
    if (rc) return rc;
    if (!d_iq || !d_audio) return fail(FSEA_EINVAL, "NULL buffer");
    if (((uintptr_t)d_iq & 1) || ((uintptr_t)d_audio & 7)) {
        return fail(FSEA_EINVAL, "d_iq must be 2-byte and d_audio 8-byte aligned");
    }
    if (n_samples == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(d->mu);
    FSEA_ON_DEVICE(d->device);
    return demod_launch(d, DM_IN_U8, d_iq, nullptr, n_samples, flip, d_audio, static_cast<hipStream_t>(stream));
}

int fsea_demod_u8_host(fsea_demod *d, const uint8_t *iq, size_t n_samples, int flip, double *audio) {
    return demod_host(d, DM_IN_U8, iq, nullptr, n_samples, flip, audio);
}

int fsea_demod_f64_host(fsea_demod *d, const double *i, const double *q, size_t n_samples, double *audio) {
    return demod_host(d, DM_IN_F64, i, q, n_samples, 0, audio);
}

}  // extern "C"
