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
// shifter's buffer, filtered in the same launch.  The conversions and the rotation live in fsea_fir_stage.h, shared with
// the decimating kernel of fsea_zoom.hip.
#include "fsea_internal.h"

#include <cmath>
#include <cstring>
#include <new>

#include "fsea_fir_stage.h"

using fsea::cf;
using fsea::cf2;
using fsea_detail::DeviceGuard;
using fsea_detail::fail;
using namespace fsea_stage;

namespace {

constexpr int FIR_WG = 256;                   // lanes per workgroup
constexpr int FIR_R = 8;                      // outputs per lane = samples per LDS row
constexpr int FIR_T = FIR_WG * FIR_R;         // outputs per workgroup
constexpr int FIR_ROW = FIR_R + 2;            // LDS row pitch in complex samples: 80 bytes, conflict-free b128 reads
constexpr int FIR_MAX_BLOCKS = FSEA_FIR_MAX_TAPS / FIR_R;
constexpr int FIR_ROWS = FIR_WG + FIR_MAX_BLOCKS;         // rows staged per tile at the largest L
constexpr int FIR_TAPS_ALLOC = FSEA_FIR_MAX_TAPS + 2 * FIR_R;  // padded taps on the device (zeros past L)
static_assert(FSEA_FIR_MAX_TAPS % FIR_R == 0, "the tap cap is a whole number of rows");

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
        stage_group<KIND, ROT>(in, s, n_in, flip, tail_in, L, rot, v);
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
    FirState state;                    // FIR_TAPS_ALLOC floats of taps, the two tails
    std::mutex mu;
    fsea_detail::HostStaging staging;  // the host-buffer forms
};

namespace {

// one launch; the caller holds f->mu and is on f's device.  rot != nullptr: the shifted u8 kernel, n includes the zero
// samples past rot->n_in
int fir_launch(fsea_fir *f, int kind, const void *d_in, size_t n, int flip, void *d_out, hipStream_t s,
               const FirRot *rot = nullptr) {
    const unsigned grid = (unsigned)((n + FIR_T - 1) / FIR_T);
    const cf *tin = f->state.in();
    cf *tout = f->state.out();
    const float *taps = f->state.taps.ptr;
    const long long nn = (long long)n;
    const uint32_t fm = (kind == FIR_IN_U8 && flip) ? 0x80808080u : 0u;
    if (rot) {
        hipLaunchKernelGGL(fsea_shift_fir_u8, dim3(grid), dim3(FIR_WG), 0, s, d_in, nn, fm, tin, tout, taps, f->n_taps,
                           static_cast<cf *>(d_out), *rot);
    } else if (kind == FIR_IN_U8) {
        hipLaunchKernelGGL(fsea_fir_u8, dim3(grid), dim3(FIR_WG), 0, s, d_in, nn, fm, tin, tout, taps, f->n_taps,
                           static_cast<cf *>(d_out));
    } else {
        hipLaunchKernelGGL(fsea_fir_f64, dim3(grid), dim3(FIR_WG), 0, s, d_in, nn, fm, tin, tout, taps, f->n_taps,
                           static_cast<cf *>(d_out));
    }
    FSEA_HIP(hipGetLastError());
    f->state.advance();
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
    if (int rc = FirState::check_taps(taps, n_taps)) return rc;
    return fsea_detail::create_object(out, device, "fsea_fir_create", [&](fsea_fir *f) {
        f->n_taps = n_taps;
        return f->state.create(taps, n_taps, FIR_TAPS_ALLOC, FSEA_FIR_MAX_TAPS);
    });
}

int fsea_fir_destroy(fsea_fir *f) { return fsea_detail::destroy_object(f); }

int fsea_fir_reset(fsea_fir *f) {
    return fsea_detail::reset_object(f, "fir is NULL", [&] { return f->state.reset(); });
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
    if (shift) {   // the n_in samples of the input have stream positions; the zeros behind them have none
        int rc = check_shift(shift->cycles_per_sample, shift->phase0_cycles, shift->sample_offset, n_in);
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
