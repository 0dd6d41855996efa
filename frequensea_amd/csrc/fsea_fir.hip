// fsea_fir.hip -- streaming complex FIR filter with real f32 taps (include/fsea.h: fsea_fir_*), the batched form of the
// reference's nrf_iq_filter: I and Q filtered independently by the same taps, the last L - 1 input samples carried from call
// to call.  Output i of a call is
//   y[i] = sum_{k < L} c[k] x_ext[i + k],   x_ext = tail ++ x,
// and the tail becomes the last L - 1 values of x_ext.
//
// Kernel ("The IQ low-pass filter"): one workgroup of 256 lanes per tile of FIR_T = 2048 outputs.  The tile's
// FIR_T + L - 1 inputs are converted once (u8 / 256 or f64 -> f32 complex) and staged in LDS as rows of FIR_R = 8
// samples, padded to 80 bytes so that the ds_read_b128 row reads of 64 lanes hit every bank once.  Lane l owns the
// FIR_R consecutive outputs l*FIR_R .. l*FIR_R + 7 and slides a register window of two rows along the taps: one row
// (four ds_read_b128) feeds 64 v_pk_fma_f32, each an (I, Q) pair times a tap broadcast from an SGPR pair.  The outputs
// go back through the same LDS rows so that the stores are coalesced.  The taps are
// zero-padded to whole rows on the device; they arrive by scalar loads.  The tail lives in two device buffers used in
// turn: a launch reads one and workgroup 0 writes the next one, so no workgroup can overwrite the old tail while the
// first tile still reads it.
//
// fsea_shift_fir_u8 (fsea_fir_u8_shifted_*) is the u8 kernel with nrf_freq_shifter fused into the staging step: every input
// sample is rotated once on its way into LDS, x = (u8 / 256) e^{2 pi i phase(P)} + 0.5 (1 + i), P its position in the
// stream.  The phasor of P is base(P & ~7) * step[P & 7]: the base from the phase reduced in double (delta * P as an exact
// two-term product) and evaluated by one sincospif, the eight steps e^{2 pi i delta j} from the kernel arguments.  A
// staged group of eight samples needs two bases at most (one when the call starts on a multiple of eight), and every
// rounding of the products is spelled out, so a sample's value depends on (delta, phase0, P) alone: the tail, the tiles and
// calls cut anywhere all see the same bits.  Samples past the input (n_in <= m < n) are plain 0.0: the zero half of the
// shifter's buffer, filtered in the same launch.
#include "fsea_internal.h"

#include <cmath>
#include <cstring>
#include <new>

#include "fsea_pk_asm.h"

using fsea::cf;
using fsea::cf2;
using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int FIR_WG = 256;                   // lanes per workgroup
constexpr int FIR_R = 8;                      // outputs per lane = samples per LDS row
constexpr int FIR_T = FIR_WG * FIR_R;         // outputs per workgroup
constexpr int FIR_ROW = FIR_R + 2;            // LDS row pitch in complex samples: 80 bytes, conflict-free b128 reads
constexpr int FIR_MAX_BLOCKS = FSEA_FIR_MAX_TAPS / FIR_R;
constexpr int FIR_ROWS = FIR_WG + FIR_MAX_BLOCKS;         // rows staged per tile at the largest L
constexpr int FIR_TAPS_ALLOC = FSEA_FIR_MAX_TAPS + 2 * FIR_R;  // padded taps on the device (zeros past L)
static_assert(FSEA_FIR_MAX_TAPS % FIR_R == 0, "the tap cap is a whole number of rows");

enum { FIR_IN_U8 = 0, FIR_IN_F64 = 1 };
constexpr double FIR_MAX_CYCLES = 1048576.0;               // |cycles_per_sample| the shifted forms accept
constexpr uint64_t FIR_MAX_POSITION = (uint64_t)1 << 52;   // stream positions stay exact as doubles

// The frequency shift of one launch (fsea_shift_fir_u8), by value in the kernel arguments.
struct FirRot {
    double delta;      // cycles per sample
    double phase0;     // phase0_cycles reduced to [0, 1)
    long long offset;  // stream position of the call's sample 0
    long long n_in;    // samples the input holds; samples n_in .. n - 1 of the call are plain 0.0
    cf step[8];        // e^{2 pi i delta j}, j < 8, rounded from double
};

// acc + w * tap, the tap broadcast from the low (even k) or the high (odd k) half of an SGPR pair
__device__ __forceinline__ cf pk_tap_fma_lo(cf w, cf taps, cf acc) {
    cf t;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(t) : "v"(w), "s"(taps), "v"(acc));
    return t;
}
__device__ __forceinline__ cf pk_tap_fma_hi(cf w, cf taps, cf acc) {
    cf t;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(t) : "v"(w), "s"(taps), "v"(acc));
    return t;
}

// e^{2 pi i (phase0 + delta P)} for a stream position P: delta * P is the exact sum of the rounded product and its fma
// residual, so the reduced phase is good to ~2^-50 turns whatever P (P < 2^52 is exact as a double); float only then
__device__ __forceinline__ cf rot_base(const FirRot &r, long long P) {
    const double k = (double)P;
    const double hi = __dmul_rn(r.delta, k);
    const double lo = fma(r.delta, k, -hi);
    double t = (hi - floor(hi)) + (lo + r.phase0);
    t -= floor(t);
    float s, c;
    sincospif(2.0f * (float)t, &s, &c);
    return cf{c, s};
}

// r.step[j] without indexing the kernel arguments by a lane's value (that would move them to scratch)
__device__ __forceinline__ cf rot_step(const FirRot &r, int j) {
    cf w = r.step[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) w = (j == i) ? r.step[i] : w;
    return w;
}

// a * b with every rounding spelled out: the same bits wherever it is inlined
__device__ __forceinline__ cf rot_mul(cf a, cf b) {
    return cf{__fmaf_rn(a[0], b[0], -__fmul_rn(a[1], b[1])), __fmaf_rn(a[0], b[1], __fmul_rn(a[1], b[0]))};
}

// the shifter's output for the sample u = u8 / 256 at a position whose phasor is ph
__device__ __forceinline__ cf rot_sample(cf u, cf ph) {
    const cf p = rot_mul(u, ph);
    return cf{__fadd_rn(p[0], 0.5f), __fadd_rn(p[1], 0.5f)};
}

template <int KIND>
__device__ __forceinline__ cf load_sample(const void *__restrict__ in, long long s, uint32_t flip) {
    if (KIND == FIR_IN_U8) {
        const uint32_t b = ((uint32_t)(static_cast<const uint16_t *>(in))[s] ^ flip) & 0xffffu;
        return cf{(float)(b & 0xffu) * (1.0f / 256.0f), (float)(b >> 8) * (1.0f / 256.0f)};
    } else {
        const double2 d = (static_cast<const double2 *>(in))[s];
        return cf{(float)d.x, (float)d.y};
    }
}

// eight consecutive samples from s (a multiple of 8, all inside the input)
template <int KIND>
__device__ __forceinline__ void load_group(const void *__restrict__ in, long long s, uint32_t flip, cf v[8]) {
    if (KIND == FIR_IN_U8) {
        const uint4 q = (static_cast<const uint4 *>(in))[s >> 3];
        const uint32_t w[4] = {q.x ^ flip, q.y ^ flip, q.z ^ flip, q.w ^ flip};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = cf{(float)(w[j] & 0xffu), (float)((w[j] >> 8) & 0xffu)} * (1.0f / 256.0f);
            v[2 * j + 1] = cf{(float)((w[j] >> 16) & 0xffu), (float)(w[j] >> 24)} * (1.0f / 256.0f);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = load_sample<KIND>(in, s + j, flip);
    }
}

__device__ __forceinline__ void read_row(const cf *row, cf v[FIR_R]) {
#pragma unroll
    for (int j = 0; j < FIR_R; j += 2) {
        const cf2 q = *reinterpret_cast<const cf2 *>(row + j);
        v[j] = cf{q[0], q[1]};
        v[j + 1] = cf{q[2], q[3]};
    }
}

// acc[r] += sum_{i < FIR_R} t[i] * win[r + i], win = a ++ b (two consecutive rows), t = taps kb*FIR_R .. + FIR_R - 1
__device__ __forceinline__ void fma_block(cf acc[FIR_R], const cf a[FIR_R], const cf b[FIR_R], const cf *__restrict__ taps2,
                                          int kb) {
    cf t[FIR_R / 2];
#pragma unroll
    for (int j = 0; j < FIR_R / 2; ++j) t[j] = taps2[kb * (FIR_R / 2) + j];
#pragma unroll
    for (int i = 0; i < FIR_R; ++i) {
#pragma unroll
        for (int r = 0; r < FIR_R; ++r) {
            const cf w = (r + i < FIR_R) ? a[r + i] : b[r + i - FIR_R];
            acc[r] = (i & 1) ? pk_tap_fma_hi(w, t[i >> 1], acc[r]) : pk_tap_fma_lo(w, t[i >> 1], acc[r]);
        }
    }
}

// sample s of the call (0 <= s < n) as the filter sees it
template <int KIND, bool ROT>
__device__ __forceinline__ cf load_input(const void *__restrict__ in, long long s, uint32_t flip, const FirRot &rot) {
    if constexpr (ROT) {
        if (s >= rot.n_in) return cf{0.0f, 0.0f};
        const long long P = rot.offset + s;
        return rot_sample(load_sample<KIND>(in, s, flip), rot_mul(rot_base(rot, P & ~7LL), rot_step(rot, (int)(P & 7))));
    } else {
        return load_sample<KIND>(in, s, flip);
    }
}

template <int KIND, bool ROT = false>
__device__ __forceinline__ void fir_body(const void *__restrict__ in, long long n, uint32_t flip, const cf *__restrict__ tail_in,
                                         cf *__restrict__ tail_out, const float *__restrict__ taps, int L, cf *__restrict__ out,
                                         const FirRot &rot = FirRot{}) {
    const long long n_in = ROT ? rot.n_in : n;   // input samples behind `in`
    __shared__ __attribute__((aligned(16))) cf lds[FIR_ROWS * FIR_ROW];
    const int tid = threadIdx.x;
    const int nb = (L + FIR_R - 1) / FIR_R;      // tap rows (zero-padded past L)
    const int span = (FIR_WG + nb) * FIR_R;      // x_ext entries the tile reads
    const long long i0 = (long long)blockIdx.x * FIR_T;  // first output = first x_ext index of the tile
    const long long s_first = i0 - (L - 1);      // input sample of x_ext[i0] (negative: the tail)
    const long long s_al = s_first & ~7LL;       // the 8-sample group it lies in
    const int groups = (int)((s_first - s_al + span + 7) >> 3);

    // stage: x_ext[i0 + i], i < span, converted to f32 complex; past the end of the input: zeros (they meet zero taps or
    // feed outputs that are not stored)
    for (int g = tid; g < groups; g += FIR_WG) {
        const long long s = s_al + 8LL * g;
        cf v[8];
        if (s >= 0 && s + 8 <= n_in) {
            load_group<KIND>(in, s, flip, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long ss = s + j;
                v[j] = ss < 0 ? (ss + (L - 1) >= 0 ? tail_in[ss + (L - 1)] : cf{0.0f, 0.0f})
                              : (ss < n_in ? load_sample<KIND>(in, ss, flip) : cf{0.0f, 0.0f});
            }
        }
        if constexpr (ROT) {
            // the group's input samples (the tail is rotated already, zeros stay zeros): stream positions P0 + j, in one
            // block of eight or two
            if (s >= 0 && s < n_in) {
                const long long P0 = rot.offset + s;
                const int o = (int)(rot.offset & 7);   // == P0 & 7: s is a multiple of 8
                const cf b0 = rot_base(rot, P0 - o);
                const cf b1 = o ? rot_base(rot, P0 - o + 8) : b0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const cf ph = rot_mul(o + j < 8 ? b0 : b1, rot_step(rot, (o + j) & 7));
                    if (s + j < n_in) v[j] = rot_sample(v[j], ph);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long long i = s + j - s_first;
            if (i >= 0 && i < span) lds[(int)(i >> 3) * FIR_ROW + (int)(i & 7)] = v[j];
        }
    }
    __syncthreads();

    const cf *taps2 = reinterpret_cast<const cf *>(taps);   // tap pairs, one SGPR pair each
    const cf *row = lds + tid * FIR_ROW;
    cf acc[FIR_R], lo[FIR_R], hi[FIR_R];
#pragma unroll
    for (int r = 0; r < FIR_R; ++r) acc[r] = cf{0.0f, 0.0f};
    read_row(row, lo);
    int b = 0;
    for (; b + 2 <= nb; b += 2) {
        read_row(row + (b + 1) * FIR_ROW, hi);
        fma_block(acc, lo, hi, taps2, b);
        read_row(row + (b + 2) * FIR_ROW, lo);
        fma_block(acc, hi, lo, taps2, b + 1);
    }
    if (b < nb) {
        read_row(row + (b + 1) * FIR_ROW, hi);
        fma_block(acc, lo, hi, taps2, b);
    }

    // store through LDS: lane l's eight outputs go to padded row l, then every wave writes 1 KiB runs of the tile
    // (16 contiguous bytes per lane) instead of 64-byte-strided pieces
    __syncthreads();  // every lane is done with the staged input
#pragma unroll
    for (int r = 0; r < FIR_R; r += 2) {
        *reinterpret_cast<cf2 *>(lds + tid * FIR_ROW + r) = cf2{acc[r][0], acc[r][1], acc[r + 1][0], acc[r + 1][1]};
    }
    __syncthreads();
    const long long left = n - i0;  // outputs of this tile still inside the call
#pragma unroll
    for (int q = 0; q < FIR_T / (2 * FIR_WG); ++q) {
        const int p = 2 * tid + 2 * FIR_WG * q;  // tile position of this lane's pair
        const cf2 v = *reinterpret_cast<const cf2 *>(lds + (p >> 3) * FIR_ROW + (p & 7));
        if (p + 2 <= left) {
            *reinterpret_cast<cf2 *>(out + i0 + p) = v;
        } else if (p < left) {
            out[i0 + p] = cf{v[0], v[1]};
        }
    }

    // the next call's tail: x_ext[n + m], m < L - 1 -- from the old tail while n + m < L - 1 (a call shorter than the tail)
    if (blockIdx.x == 0) {
        for (int m = tid; m < L - 1; m += FIR_WG) {
            const long long e = n + m;
            tail_out[m] = e < L - 1 ? tail_in[e] : load_input<KIND, ROT>(in, e - (L - 1), flip, rot);
        }
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(FIR_WG) void fsea_fir_u8(const void *__restrict__ in, long long n, uint32_t flip,
                                                                  const cf *__restrict__ tail_in, cf *__restrict__ tail_out,
                                                                  const float *__restrict__ taps, int L, cf *__restrict__ out) {
    fir_body<FIR_IN_U8>(in, n, flip, tail_in, tail_out, taps, L, out);
}

extern "C" __global__ __launch_bounds__(FIR_WG) void fsea_fir_f64(const void *__restrict__ in, long long n, uint32_t flip,
                                                                   const cf *__restrict__ tail_in, cf *__restrict__ tail_out,
                                                                   const float *__restrict__ taps, int L, cf *__restrict__ out) {
    fir_body<FIR_IN_F64>(in, n, flip, tail_in, tail_out, taps, L, out);
}

// the u8 kernel with the frequency shift in its staging step
extern "C" __global__ __launch_bounds__(FIR_WG) void fsea_shift_fir_u8(const void *__restrict__ in, long long n, uint32_t flip,
                                                                        const cf *__restrict__ tail_in, cf *__restrict__ tail_out,
                                                                        const float *__restrict__ taps, int L, cf *__restrict__ out,
                                                                        FirRot rot) {
    fir_body<FIR_IN_U8, true>(in, n, flip, tail_in, tail_out, taps, L, out, rot);
}

struct fsea_fir {
    int n_taps = 0;
    int device = 0;
    float *d_taps = nullptr;       // FIR_TAPS_ALLOC floats, zeros past n_taps
    cf *d_tail[2] = {nullptr, nullptr};  // FSEA_FIR_MAX_TAPS samples each; d_tail[cur] is the current tail
    int cur = 0;
    std::mutex mu;
    fsea_detail::HostStaging staging;  // the host-buffer forms

    ~fsea_fir() {
        if (d_taps) (void)hipFree(d_taps);
        for (cf *tail : d_tail)
            if (tail) (void)hipFree(tail);
    }
};

namespace {

// What the shifted kernel needs for a call whose sample 0 is at stream position `offset`, n_in samples behind its input.
FirRot make_rot(double cycles_per_sample, double phase0_cycles, uint64_t offset, size_t n_in) {
    FirRot r;
    r.delta = cycles_per_sample;
    r.phase0 = phase0_cycles - std::floor(phase0_cycles);
    r.offset = (long long)offset;
    r.n_in = (long long)n_in;
    for (int j = 0; j < 8; ++j) {
        double t = cycles_per_sample * j;
        t -= std::floor(t);
        r.step[j] = cf{(float)std::cos(2.0 * M_PI * t), (float)std::sin(2.0 * M_PI * t)};
    }
    return r;
}

int check_shift(double cycles_per_sample, double phase0_cycles, uint64_t offset, size_t n) {
    if (!(std::fabs(cycles_per_sample) <= FIR_MAX_CYCLES) || !std::isfinite(phase0_cycles)) {
        return fail(FSEA_EINVAL, "cycles_per_sample must be finite and within +-%g, phase0_cycles finite", FIR_MAX_CYCLES);
    }
    if (offset > FIR_MAX_POSITION || n > FIR_MAX_POSITION - offset) {
        return fail(FSEA_EINVAL, "sample_offset + n_samples must not exceed 2^52");
    }
    return FSEA_OK;
}

// one launch; the caller holds f->mu and is on f's device.  rot != nullptr: the shifted u8 kernel, n includes the zero
// samples past rot->n_in
int fir_launch(fsea_fir *f, int kind, const void *d_in, size_t n, int flip, void *d_out, hipStream_t s,
               const FirRot *rot = nullptr) {
    const unsigned grid = (unsigned)((n + FIR_T - 1) / FIR_T);
    const cf *tin = f->d_tail[f->cur];
    cf *tout = f->d_tail[f->cur ^ 1];
    const long long nn = (long long)n;
    const uint32_t fm = (kind == FIR_IN_U8 && flip) ? 0x80808080u : 0u;
    if (rot) {
        hipLaunchKernelGGL(fsea_shift_fir_u8, dim3(grid), dim3(FIR_WG), 0, s, d_in, nn, fm, tin, tout, f->d_taps, f->n_taps,
                           static_cast<cf *>(d_out), *rot);
    } else if (kind == FIR_IN_U8) {
        hipLaunchKernelGGL(fsea_fir_u8, dim3(grid), dim3(FIR_WG), 0, s, d_in, nn, fm, tin, tout, f->d_taps, f->n_taps,
                           static_cast<cf *>(d_out));
    } else {
        hipLaunchKernelGGL(fsea_fir_f64, dim3(grid), dim3(FIR_WG), 0, s, d_in, nn, fm, tin, tout, f->d_taps, f->n_taps,
                           static_cast<cf *>(d_out));
    }
    FSEA_HIP(hipGetLastError());
    f->cur ^= 1;
    return FSEA_OK;
}

// the host-buffer forms: one launch through the object's staging (fsea_detail::HostStaging)
int fir_host(fsea_fir *f, int kind, const void *in, size_t n, int flip, float *out, const FirRot *rot = nullptr) {
    if (!f) return fail(FSEA_EINVAL, "fir is NULL");
    if (n == 0) return FSEA_OK;
    if (!in || !out) return fail(FSEA_EINVAL, "NULL buffer");
    if (n > ((size_t)1 << 40)) return fail(FSEA_EINVAL, "n_samples %zu too large", n);
    std::lock_guard<std::mutex> lock(f->mu);
    FSEA_ON_DEVICE(f->device);
    const size_t in_bytes = n * (kind == FIR_IN_U8 ? 2 : 16);
    return f->staging.run(
        in_bytes, n * sizeof(cf), out, [&](void *h_in) { std::memcpy(h_in, in, in_bytes); },
        [&](void *d_in, void *d_out, hipStream_t s) { return fir_launch(f, kind, d_in, n, flip, d_out, s, rot); });
}

}  // namespace

extern "C" {

int fsea_fir_lowpass_taps(double sample_rate, double half_ampl_freq, int length, double *taps) {
#pragma clang fp contract(off)
    // the reference's window-method design, operation for operation (no fused multiply-adds): bit-exact in double
    if (!taps) return fail(FSEA_EINVAL, "taps is NULL");
    if (length < 1) return fail(FSEA_EINVAL, "length must be >= 1, got %d", length);
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate) || !std::isfinite(half_ampl_freq)) {
        return fail(FSEA_EINVAL, "sample_rate must be positive and finite, half_ampl_freq finite");
    }
    const double two_pi = M_PI * 2;
    const int m = length + (length + 1) % 2;     // an even length is designed one tap longer
    const double f = half_ampl_freq / sample_rate;
    const int c = m / 2;
    double *v = new (std::nothrow) double[m];
    if (!v) return fail(FSEA_ENOMEM, "out of host memory");
    double sum = 0.0;
    for (int i = 0; i < m; ++i) {
        double x;
        if (i == c) {
            x = two_pi * f;
        } else {
            const double a = two_pi * (i + 1) / (double)(m + 1);
            x = sin(two_pi * f * (i - c)) / (double)(i - c);
            x *= 0.42 - 0.5 * cos(a) + 0.08 * cos(2 * a);
        }
        sum += x;
        v[i] = x;
    }
    for (int i = 0; i < length; ++i) taps[i] = v[i] / sum;   // the first `length` of the m taps
    delete[] v;
    return FSEA_OK;
}

int fsea_fir_create(fsea_fir **out, const double *taps, int n_taps, int device) {
    if (!out) return fail(FSEA_EINVAL, "fir out-pointer is NULL");
    *out = nullptr;
    if (!taps) return fail(FSEA_EINVAL, "taps is NULL");
    if (n_taps < 1 || n_taps > FSEA_FIR_MAX_TAPS) {
        return fail(FSEA_EINVAL, "n_taps must be in [1, %d], got %d", FSEA_FIR_MAX_TAPS, n_taps);
    }
    for (int k = 0; k < n_taps; ++k) {
        if (!std::isfinite(taps[k])) return fail(FSEA_EINVAL, "tap %d is not finite", k);
    }
    return fsea_detail::create_object(out, device, "fsea_fir_create", [&](fsea_fir *f) {
        f->n_taps = n_taps;
        float tf[FIR_TAPS_ALLOC] = {};
        for (int k = 0; k < n_taps; ++k) tf[k] = (float)taps[k];
        hipError_t e = hipMalloc(&f->d_taps, sizeof(tf));
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(&f->d_tail[i], FSEA_FIR_MAX_TAPS * sizeof(cf));
        if (e == hipSuccess) e = hipMemcpy(f->d_taps, tf, sizeof(tf), hipMemcpyHostToDevice);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMemset(f->d_tail[i], 0, FSEA_FIR_MAX_TAPS * sizeof(cf));
        return e;
    });
}

int fsea_fir_destroy(fsea_fir *f) { return fsea_detail::destroy_object(f); }

int fsea_fir_reset(fsea_fir *f) {
    if (!f) return fail(FSEA_EINVAL, "fir is NULL");
    std::lock_guard<std::mutex> lock(f->mu);
    FSEA_ON_DEVICE(f->device);
    FSEA_HIP(hipDeviceSynchronize());
    FSEA_HIP(hipMemset(f->d_tail[f->cur], 0, FSEA_FIR_MAX_TAPS * sizeof(cf)));
    FSEA_HIP(hipDeviceSynchronize());
    return FSEA_OK;
}

int fsea_fir_n_taps(const fsea_fir *f) { return f ? f->n_taps : 0; }

int fsea_fir_u8_device(fsea_fir *f, const void *d_iq, size_t n_samples, int flip, void *d_out, void *stream) {
    if (!f) return fail(FSEA_EINVAL, "fir is NULL");
    if (n_samples == 0) return FSEA_OK;
    if (!d_iq || !d_out) return fail(FSEA_EINVAL, "NULL buffer");
    if (int rc = fsea_detail::check_aligned16("d_iq and d_out", d_iq, d_out)) return rc;
    if (n_samples > ((size_t)1 << 40)) return fail(FSEA_EINVAL, "n_samples %zu too large", n_samples);
    std::lock_guard<std::mutex> lock(f->mu);
    FSEA_ON_DEVICE(f->device);
    return fir_launch(f, FIR_IN_U8, d_iq, n_samples, flip, d_out, static_cast<hipStream_t>(stream));
}

int fsea_fir_u8_host(fsea_fir *f, const uint8_t *iq, size_t n_samples, int flip, float *out) {
    return fir_host(f, FIR_IN_U8, iq, n_samples, flip, out);
}

int fsea_fir_u8_shifted_device(fsea_fir *f, const void *d_iq, size_t n_samples, int flip, double cycles_per_sample,
                               double phase0_cycles, uint64_t sample_offset, void *d_out, void *stream) {
    const fsea_detail::FirShift shift = {cycles_per_sample, phase0_cycles, sample_offset};
    return fsea_detail::fir_launch_device(f, 0, d_iq, n_samples, 0, flip, &shift, d_out, static_cast<hipStream_t>(stream));
}

int fsea_fir_u8_shifted_host(fsea_fir *f, const uint8_t *iq, size_t n_samples, int flip, double cycles_per_sample,
                             double phase0_cycles, uint64_t sample_offset, float *out) {
    if (!f) return fail(FSEA_EINVAL, "fir is NULL");
    int rc = check_shift(cycles_per_sample, phase0_cycles, sample_offset, n_samples);
    if (rc) return rc;
    const FirRot rot = make_rot(cycles_per_sample, phase0_cycles, sample_offset, n_samples);
    return fir_host(f, FIR_IN_U8, iq, n_samples, flip, out, &rot);
}

int fsea_fir_f64_host(fsea_fir *f, const double *iq, size_t n_samples, float *out) {
    return fir_host(f, FIR_IN_F64, iq, n_samples, 0, out);
}

}  // extern "C"

int fsea_detail::fir_launch_device(fsea_fir *f, int f64, const void *d_in, size_t n_in, size_t n_zero, int flip,
                                   const FirShift *shift, void *d_out, hipStream_t s) {
    if (!f) return fail(FSEA_EINVAL, "fir is NULL");
    if (shift && f64) return fail(FSEA_EINVAL, "the frequency shift takes 8-bit input");
    if (n_zero && !shift) return fail(FSEA_EINVAL, "zero samples follow a shifted block only");
    if (n_in > ((size_t)1 << 40) || n_zero > ((size_t)1 << 40)) return fail(FSEA_EINVAL, "n_samples %zu too large", n_in);
    const size_t n = n_in + n_zero;
    if (shift) {
        int rc = check_shift(shift->cycles_per_sample, shift->phase0_cycles, shift->sample_offset, n);
        if (rc) return rc;
    }
    if (n == 0) return FSEA_OK;
    if ((n_in && !d_in) || !d_out) return fail(FSEA_EINVAL, "NULL buffer");
    if (int rc = fsea_detail::check_aligned16("d_iq and d_out", d_in, d_out)) return rc;
    std::lock_guard<std::mutex> lock(f->mu);
    FSEA_ON_DEVICE(f->device);
    if (!shift) return fir_launch(f, f64 ? FIR_IN_F64 : FIR_IN_U8, d_in, n, flip, d_out, s);
    const FirRot rot = make_rot(shift->cycles_per_sample, shift->phase0_cycles, shift->sample_offset, n_in);
    return fir_launch(f, FIR_IN_U8, d_in, n, flip, d_out, s, &rot);
}
