// fsea_fir_stage.h -- how an input sample becomes the f32 complex value a FIR kernel stages in LDS, shared by the kernels of
// fsea_fir.hip (fsea_fir_u8, fsea_fir_f64, fsea_shift_fir_u8), fsea_zoom.hip (fsea_shift_decim_u8), fsea_extract.hip
// (fsea_extract_u8) and fsea_pfb.hip (fsea_pfb_frames_u8): the byte and f64 conversions, the frequency shift of
// fsea_fir_u8_shifted_* (include/fsea.h) with every rounding spelled out, the packed tap FMA, the host side of the shift
// (FirRot from the caller's arguments, the argument limits), and the filter state the three objects carry from call to call
// (FirState: the taps and two tails of a length each object gives at create).  A sample's value is a function of
// (cycles_per_sample, phase0_cycles, stream position) alone, so every kernel that stages through these helpers sees the
// same bits.
#pragma once

#include "fsea_internal.h"

#include <cmath>
#include <vector>

#include "fsea_pk_asm.h"

namespace fsea_stage {

using fsea::cf;
using fsea::cf2;

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
// the same with a tap pair of the lane's own in a VGPR pair (fsea_pfb.hip: every column has its own branch of the prototype)
__device__ __forceinline__ cf pk_tap_fma_lo_v(cf w, cf taps, cf acc) {
    cf t;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(t) : "v"(w), "v"(taps), "v"(acc));
    return t;
}
__device__ __forceinline__ cf pk_tap_fma_hi_v(cf w, cf taps, cf acc) {
    cf t;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(t) : "v"(w), "v"(taps), "v"(acc));
    return t;
}

// e^{2 pi i (phase0 + delta P)} for a stream position P <= 2^52 (exact as a double): delta * P is the exact sum of the
// rounded product hi and its fma residual lo.  hi is reduced modulo 1 exactly; lo is added to phase0 as it is, |lo| <=
// ulp(hi) / 2.  While |delta P| < 2^53 (|delta| <= 0.5 at every P) lo is below 1 and the reduced phase is within about
// 2^-50 turns of the exact one (measured: 2^-52).  Beyond that lo grows to 2^19 at |delta| = 2^20, P = 2^52, and the two
// sums round at its size: no worse than 2^-35 turns by that argument, 2^-36 measured (DESIGN.md section 6,
// tests/test_shift_ref_host.py, which holds this arithmetic to 2^-30).  The float conversion that follows rounds to 2^-25.
// No contraction in here: device code is compiled with -ffp-contract=fast, __dmul_rn is a plain multiplication to the
// compiler, and hi - floor(hi) was fused into fma(delta, k, -floor(hi)) -- the fraction of the EXACT product, to which lo
// was then added a second time: an error of lo, that of one rounded product (tests/test_gpu_shift_domain.py found it).
__device__ __forceinline__ cf rot_base(const FirRot &r, long long P) {
#pragma clang fp contract(off)
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

// One staged group: the eight samples s .. s + 7 of a call (s a multiple of 8, negative in the tail) as the filter sees
// them.  tail_in holds the L - 1 samples in front of the call (rotated already); past the n_in samples of the input: 0.0.
template <int KIND, bool ROT>
__device__ __forceinline__ void stage_group(const void *in, long long s, long long n_in, uint32_t flip, const cf *tail_in, int L,
                                            const FirRot &rot, cf v[8]) {
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
}

// stage_group for a job that begins anywhere in a resident buffer (fsea_extract_u8): sample 0 of the job is element `first`
// of `in`, the job has n samples, and the group is aligned to the buffer, not to the job: first + s is a multiple of 8, s
// itself any number from -7 on.  The samples in front of the job are 0.0 (a zero tail) and so are those behind it; no load
// leaves [first, first + n).  The stream position of sample s is rot.offset + s, and a sample's phasor is rot_base at
// P & ~7 times step P & 7 as in stage_group: the same bits whatever the grouping.  o = P0 & 7 is the same for every group
// of a job, the groups being eight samples apart, so the caller works it out once, from uniform values, and hands in the
// steps in the group's order: turned[j] = step[(o + j) & 7], eight scalar loads at a uniform index.  (That kernel reads its
// FirRot from device memory, not from its arguments; rot_step's selects among eight loaded values the compiler made a
// table in scratch, indexed by the lane's o + j, or by the uniform one.)  Of rot only delta, phase0 and offset are read.
template <int KIND>
__device__ __forceinline__ void stage_group_at(const void *in, long long first, long long s, long long n, uint32_t flip,
                                               const FirRot &rot, const cf turned[8], int o, cf v[8]) {
    if (s >= 0 && s + 8 <= n) {
        load_group<KIND>(in, first + s, flip, v);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long long ss = s + j;
            v[j] = ss >= 0 && ss < n ? load_sample<KIND>(in, first + ss, flip) : cf{0.0f, 0.0f};
        }
    }
    if (s + 8 > 0 && s < n) {
        const long long P0 = rot.offset + s;   // P0 & 7 == o
        const cf b0 = rot_base(rot, P0 - o);   // in front of position 0 only for samples in front of the job: not used
        const cf b1 = o ? rot_base(rot, P0 - o + 8) : b0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const cf ph = rot_mul(o + j < 8 ? b0 : b1, turned[j]);
            if (s + j >= 0 && s + j < n) v[j] = rot_sample(v[j], ph);
        }
    }
}

// What the shifted kernel needs for a call whose sample 0 is at stream position `offset`, n_in samples behind its input.
inline FirRot make_rot(double cycles_per_sample, double phase0_cycles, uint64_t offset, size_t n_in) {
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

inline int check_shift(double cycles_per_sample, double phase0_cycles, uint64_t offset, size_t n) {
    if (!(std::fabs(cycles_per_sample) <= FIR_MAX_CYCLES)) {
        return fsea_detail::fail(FSEA_EINVAL, "cycles_per_sample must be finite and within +-%g", FIR_MAX_CYCLES);
    }
    if (!std::isfinite(phase0_cycles)) return fsea_detail::fail(FSEA_EINVAL, "phase0_cycles must be finite");
    if (offset > FIR_MAX_POSITION || n > FIR_MAX_POSITION - offset) {
        return fsea_detail::fail(FSEA_EINVAL, "sample_offset + n_samples must not exceed 2^52");
    }
    return FSEA_OK;
}

// What fsea_fir, fsea_zoom and fsea_pfb keep between calls: the taps as floats, padded with zeros to the length the
// object's kernel reads, and two tails of tail_len samples, the length given at create: FSEA_FIR_MAX_TAPS for the filter
// and the zoom, the bank's L - 1.  A launch reads in() and writes out(); advance() makes the written tail the current one.
struct FirState {
    fsea_detail::DeviceArray<float> taps;
    fsea_detail::DeviceArray<cf> tail[2];
    size_t tail_len = 0;
    int cur = 0;

    static int check_finite(const double *taps, int n_taps) {
        for (int k = 0; k < n_taps; ++k) {
            if (!std::isfinite(taps[k])) return fsea_detail::fail(FSEA_EINVAL, "tap %d is not finite", k);
        }
        return FSEA_OK;
    }
    static int check_taps(const double *taps, int n_taps) {
        if (!taps) return fsea_detail::fail(FSEA_EINVAL, "taps is NULL");
        if (n_taps < 1 || n_taps > FSEA_FIR_MAX_TAPS) {
            return fsea_detail::fail(FSEA_EINVAL, "n_taps must be in [1, %d], got %d", FSEA_FIR_MAX_TAPS, n_taps);
        }
        return check_finite(taps, n_taps);
    }
    hipError_t create(const double *t, int n_taps, int alloc_floats, size_t tail_samples) {
        std::vector<float> tf((size_t)alloc_floats, 0.0f);
        for (int k = 0; k < n_taps; ++k) tf[k] = (float)t[k];
        tail_len = tail_samples;
        hipError_t e = taps.upload(tf.data(), tf.size());
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = tail[i].zeros(tail_len);
        return e;
    }
    const cf *in() const { return tail[cur].ptr; }
    cf *out() const { return tail[cur ^ 1].ptr; }
    void advance() { cur ^= 1; }
    int reset() {   // the current tail only: the other one is written whole by the next launch
        FSEA_HIP(tail[cur].zero(tail_len));
        return FSEA_OK;
    }
};

}  // namespace fsea_stage
