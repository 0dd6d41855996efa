// fsea_pfb.hip -- the polyphase filter bank (include/fsea.h: fsea_pfb_*): a prototype low-pass of L = M P taps folded into M
// branches of P taps, one M-point transform of the object's own plan per frame, a frame every D = M / q samples.  A call
// reads the 8-bit stream once and leaves n / D frames of M f32 pairs resident for the plan.
//
// Kernel fsea_pfb_frames_u8 ("The polyphase filter bank"): with x_ext = tail ++ x,
//   v_t[r] = sum_{p < P} c[p M + r] x_ext[t D + p M + r],    frames[t][(r + s0 + t D) mod M] = v_t[r],    t < n / D, r < M,
// one FMA chain per output, p ascending, from +0 (output t D of the full-rate filter with the taps of branch r, as a value).
// x_ext[t D + p M + r] = x_ext[(t + p q) D + r]: tap p of frame t reads column r of the segment that starts at frame
// t + p q.  A workgroup of PF_WG = 256 lanes owns T frames x C columns: it stages the T + (2 ceil(P / 2) - 1) q segments
// x_ext[t' D + c], c in [c0, c0 + C), once in LDS through stage_group (fsea_fir_stage.h: 16-byte loads, the tail, zeros past
// the input, the filter's bits) -- a segment starts at any sample, so its first 8-sample group is aligned down as in
// fsea_shift_decim_u8 -- and then every lane owns one column: its P taps sit in P / 2 VGPR pairs, per frame it reads P
// consecutive-lane 8-byte words a fixed stride apart (row-major image, pitch C: no bank conflicts) and stores 8 bytes at
// the rotated column.  An input sample is used P q times; staging makes that one global read per workgroup.  An odd P runs
// with a zero tap behind it, on a row that is staged like the others (finite values: the chain's bits stay).
// C = 256 columns at most: at M = 16384 a frame spans 1 MiB, the chunk bounds the image.  256 / C frames are in work at a
// time.  The image is a static array in three sizes (20, 40 and 80 KiB: kernels ..._s, ..._m and the plain name: eight, four
// and two workgroups per CU); pfb_shape picks the image, C and T per (M, P, q).  Workgroup (0, 0) writes the
// next tail (L - 1 up to 262143 samples) into the second of two tail buffers.
//
// Kernel fsea_pfb_transpose: series[k F + t] = rows[t][k] for complex rows, 32 x 32 tiles through a padded LDS tile,
// 8-byte accesses contiguous along k on the read and along t on the write.
#include "fsea_fir_stage.h"

using fsea_detail::DeviceGuard;
using fsea_detail::fail;
using namespace fsea_stage;

namespace {

constexpr int PF_WG = 256;                                        // lanes per workgroup
constexpr int PF_CAP_S = 2560, PF_CAP_M = 5120, PF_CAP_L = 10240;  // samples of the three LDS images
constexpr int PF_MAX_TILE = 128;                                  // frames per workgroup at most
constexpr int PF_TR = 32;                                         // the transpose's tile
constexpr size_t PF_MAX_SAMPLES = (size_t)1 << 31;
static_assert(2 * PF_CAP_L * sizeof(cf) <= 160 * 1024, "two workgroups per CU at the largest image");

// The tile of a (M, P, q): C columns, T frames, `extra` rows of the image beyond T.
struct PfbShape {
    int C, T, extra;
};

constexpr PfbShape pfb_tile(int cap, int width, int M, int extra) {
    const int C = M < width ? M : width, slots = PF_WG / C;
    int T = cap / C - extra;
    if (T > PF_MAX_TILE) T = PF_MAX_TILE;
    if (T >= slots) T -= T % slots;
    return PfbShape{C, T, extra};
}

// The smallest image, and in it the widest chunk, whose tile is at least twice the extra rows (two thirds of the staged rows
// are the tile's own): a small image keeps more workgroups on a CU, and they hide one another's staging.  Where none has
// such a tile (P = 16 at q = 4): 64 columns in the largest.
constexpr PfbShape pfb_shape(int M, int P, int q) {
    const int extra = (2 * ((P + 1) / 2) - 1) * q;
    for (int cap : {PF_CAP_S, PF_CAP_M, PF_CAP_L}) {
        for (int width : {256, 128, 64}) {
            const PfbShape sh = pfb_tile(cap, width, M, extra);
            if (sh.T >= 1 && sh.T >= 2 * extra) return sh;
        }
    }
    return pfb_tile(PF_CAP_L, 64, M, extra);
}
static_assert(pfb_shape(FSEA_PFB_MAX_CHANNELS, FSEA_PFB_MAX_BRANCH_TAPS, 4).T >= 64, "the widest image at the longest branch");
static_assert(pfb_shape(2, 16, 4).T > 0 && pfb_shape(64, 16, 4).T > 0 && pfb_shape(256, 16, 4).T > 0, "every shape has a tile");

// The lane's column over the frames of the tile, NP tap pairs: frame t of the tile reads image rows t + p q, p < 2 NP, at
// the lane's column (col = the image at that column), and goes to `out` (frame 0 of the tile, column 0) at the rotated
// column: rot0 = (s0 + t0 D) mod M at frame 0, D more (mod M) with every frame.
template <int NP>
__device__ __forceinline__ void pfb_column(const cf *col, const float *__restrict__ taps, int M, int P, int D, int q, int C,
                                           int r, int slot, int slots, int n_tile, int rot0, cf *__restrict__ out) {
    cf tp[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        tp[j] = cf{taps[(size_t)(2 * j) * M + r], 2 * j + 1 < P ? taps[(size_t)(2 * j + 1) * M + r] : 0.0f};
    }
    const int step = q * C;
    for (int t = slot; t < n_tile; t += slots) {
        const cf *row = col + t * C;
        cf x[2 * NP];
#pragma unroll
        for (int p = 0; p < 2 * NP; ++p) x[p] = row[p * step];
        cf acc = cf{0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            acc = pk_tap_fma_lo_v(x[2 * j], tp[j], acc);
            acc = pk_tap_fma_hi_v(x[2 * j + 1], tp[j], acc);
        }
        int c = r + rot0 + (t & (q - 1)) * D;   // t D mod M = (t mod q) D, q a power of two; rot0 < M
        c -= c >= 2 * M ? 2 * M : c >= M ? M : 0;
        out[(size_t)t * M + c] = acc;
    }
}

template <int CAP>
__device__ __forceinline__ void pfb_body(const void *__restrict__ in, long long n, uint32_t flip, const cf *__restrict__ tail_in,
                                         cf *__restrict__ tail_out, const float *__restrict__ taps, int M, int P, int q, int C,
                                         int T, int s0m, cf *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) cf lds[CAP];
    const int tid = threadIdx.x;
    const int D = M / q, L = M * P;
    const int np = (P + 1) >> 1;                                   // tap pairs
    const long long n_frames = n / D;
    const long long t0 = (long long)blockIdx.x * T;                // first frame of the tile
    const long long left = n_frames - t0;                          // frames from there on (0: a call with no frame)
    const int n_tile = left < T ? (int)left : T;
    const int c0 = (int)blockIdx.y * C;                            // first column of the chunk
    const int width = M - c0 < C ? M - c0 : C;                     // its columns (the last chunk may be partial)
    const int n_rows = n_tile > 0 ? n_tile + (2 * np - 1) * q : 0; // image rows: segments t0 .. t0 + n_rows - 1
    const int gmax = (C + 14) >> 3;                                // 8-sample groups a row of C columns can touch
    const FirRot no_rot = {};                                      // not read: nothing is rotated here

    // stage: lds[j C + m] = x_ext[(t0 + j) D + c0 + m], j < n_rows, m < width.  A group past the input or in front of the
    // tail stages zeros; every entry a stored output multiplies by a tap of the prototype lies inside the tail or the input.
    for (int item = tid; item < n_rows * gmax; item += PF_WG) {
        const int j = item / gmax, g = item - j * gmax;
        const long long s_first = (t0 + j) * D + c0 - (L - 1);     // input sample of the row's column 0 (negative: the tail)
        const long long s_al = s_first & ~7LL;                     // the 8-sample group it lies in
        const int lead = (int)(s_first - s_al);
        if (8 * g < lead + width) {
            cf v[8];
            stage_group<FIR_IN_U8, false>(in, s_al + 8LL * g, n, flip, tail_in, L, no_rot, v);
            cf *row = lds + j * C;
            const int m0 = 8 * g - lead;                           // the row's column of the group's sample 0
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if ((unsigned)(m0 + k) < (unsigned)width) row[m0 + k] = v[k];
            }
        }
    }
    __syncthreads();

    // 256 / C frames at a time, a lane per column
    const int slots = PF_WG / C;
    const int slot = tid / C, cl = tid - slot * C;
    if (slot < slots && cl < width && n_tile > 0) {
        int rot0 = s0m + (int)(t0 & (q - 1)) * D;
        rot0 -= rot0 >= M ? M : 0;
        cf *o = out + (size_t)t0 * M;
        const cf *col = lds + cl;
        const int r = c0 + cl;
        switch (np) {
#define FSEA_PFB_CASE(NP) case NP: pfb_column<NP>(col, taps, M, P, D, q, C, r, slot, slots, n_tile, rot0, o); break;
            FSEA_PFB_CASE(1) FSEA_PFB_CASE(2) FSEA_PFB_CASE(3) FSEA_PFB_CASE(4)
            FSEA_PFB_CASE(5) FSEA_PFB_CASE(6) FSEA_PFB_CASE(7) FSEA_PFB_CASE(8)
#undef FSEA_PFB_CASE
        }
    }

    // the next call's tail: x_ext[n + m], m < L - 1 -- from the old tail while n + m < L - 1 (a call shorter than the tail)
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int m = tid; m < L - 1; m += PF_WG) {
            const long long e = n + m;
            tail_out[m] = e < L - 1 ? tail_in[e] : load_sample<FIR_IN_U8>(in, e - (L - 1), flip);
        }
    }
}

}  // namespace

#define FSEA_PFB_KERNEL(name, cap)                                                                                          \
    extern "C" __global__ __launch_bounds__(PF_WG) void name(                                                               \
        const void *__restrict__ in, long long n, uint32_t flip, const cf *__restrict__ tail_in, cf *__restrict__ tail_out,  \
        const float *__restrict__ taps, int M, int P, int q, int C, int T, int s0m, cf *__restrict__ out) {                 \
        pfb_body<cap>(in, n, flip, tail_in, tail_out, taps, M, P, q, C, T, s0m, out);                                       \
    }
FSEA_PFB_KERNEL(fsea_pfb_frames_u8_s, PF_CAP_S)
FSEA_PFB_KERNEL(fsea_pfb_frames_u8_m, PF_CAP_M)
FSEA_PFB_KERNEL(fsea_pfb_frames_u8, PF_CAP_L)

// series[k F + t] = rows[t][k], t < F, k < M: a tile of 32 x 32 through LDS, a column of padding against bank conflicts
extern "C" __global__ __launch_bounds__(PF_WG) void fsea_pfb_transpose(const cf *__restrict__ rows, long long F, int M,
                                                                        cf *__restrict__ series) {
    __shared__ cf tile[PF_TR][PF_TR + 1];
    const int x = threadIdx.x & (PF_TR - 1), y0 = threadIdx.x / PF_TR;   // 32 x 8 lanes
    const long long tb = (long long)blockIdx.y * PF_TR;
    const int kb = (int)blockIdx.x * PF_TR;
    for (int y = y0; y < PF_TR; y += PF_WG / PF_TR) {
        if (tb + y < F && kb + x < M) tile[y][x] = rows[(size_t)(tb + y) * M + kb + x];
    }
    __syncthreads();
    for (int y = y0; y < PF_TR; y += PF_WG / PF_TR) {
        if (kb + y < M && tb + x < F) series[(size_t)(kb + y) * F + tb + x] = tile[x][y];
    }
}

struct fsea_pfb {
    int channels = 0, branch_taps = 0, oversampling = 1, mode = 0;
    int device = 0;
    uint64_t s0 = 0;                              // samples consumed since create or reset
    FirState state;                               // the L taps as floats, two tails of L - 1 samples
    fsea_detail::SharedScratch frames;            // the frames of the last call; its event orders the calls
    std::mutex mu;
    fsea_detail::HostStaging staging;             // the host form
    fsea_detail::Owned<fsea_plan, fsea_plan_destroy> plan;   // (M, M, mode) on the frames; the first to go
};

namespace {

size_t out_frames(const fsea_pfb *b, size_t n_samples) { return n_samples / (size_t)(b->channels / b->oversampling); }

int check_shape(int channels, int branch_taps) {
    if (channels < 2 || channels > FSEA_PFB_MAX_CHANNELS || channels % 2) {
        return fail(FSEA_EINVAL, "channels must be even and in [2, %d], got %d", FSEA_PFB_MAX_CHANNELS, channels);
    }
    if (branch_taps < 1 || branch_taps > FSEA_PFB_MAX_BRANCH_TAPS) {
        return fail(FSEA_EINVAL, "branch_taps must be in [1, %d], got %d", FSEA_PFB_MAX_BRANCH_TAPS, branch_taps);
    }
    return FSEA_OK;
}

// what a run checks before it looks into the object
int check_run(const fsea_pfb *b, const void *iq, size_t n, const void *series) {
    if (!b) return fail(FSEA_EINVAL, "pfb is NULL");
    if (series && b->mode != FSEA_MODE_COMPLEX_F32) {
        return fail(FSEA_EINVAL, "a series needs FSEA_MODE_COMPLEX_F32, the object has mode %d", b->mode);
    }
    if (n > PF_MAX_SAMPLES) return fail(FSEA_EINVAL, "n_samples %zu too large", n);
    if (n && !iq) return fail(FSEA_EINVAL, "NULL buffer");
    return FSEA_OK;
}

// and what it checks in it
int check_outputs(const fsea_pfb *b, size_t n, const void *rows) {
    const size_t F = out_frames(b, n);
    if (F * (size_t)b->channels > PF_MAX_SAMPLES) {
        return fail(FSEA_EINVAL, "%zu frames of %d channels are more than 2^31 outputs", F, b->channels);
    }
    if (F && !rows) return fail(FSEA_EINVAL, "NULL buffer for the %zu rows of the call", F);
    return FSEA_OK;
}

// One call on device buffers, asynchronous on `s`: the frames launch into the object's buffer, the plan's launch on the
// frames, the transpose and the copy of the frames where asked for.  The caller holds b->mu and is on b's device.
int queue_call(fsea_pfb *b, const void *d_iq, size_t n, int flip, void *d_rows, void *d_frames, void *d_series, hipStream_t s) {
    const int M = b->channels, P = b->branch_taps, q = b->oversampling;
    const size_t F = out_frames(b, n), n_out = F * (size_t)M;
    if (n == 0) return FSEA_OK;
    // every call, on whatever stream, follows the previous user of the frames and the tails
    int rc = b->frames.acquire(n_out * sizeof(cf) + 16, s);
    if (rc) return rc;
    cf *d_out = static_cast<cf *>(b->frames.buf.ptr);
    const PfbShape sh = pfb_shape(M, P, q);
    const int need = (sh.T + sh.extra) * sh.C;
    auto kernel = need <= PF_CAP_S ? fsea_pfb_frames_u8_s : need <= PF_CAP_M ? fsea_pfb_frames_u8_m : fsea_pfb_frames_u8;
    // no frame: one workgroup, the tail still advances
    const dim3 grid(F ? (unsigned)((F + sh.T - 1) / sh.T) : 1u, F ? (unsigned)((M + sh.C - 1) / sh.C) : 1u);
    hipLaunchKernelGGL(kernel, grid, dim3(PF_WG), 0, s, d_iq, (long long)n, flip ? 0x80808080u : 0u,
                       b->state.in(), b->state.out(), (const float *)b->state.taps.ptr, M, P, q, sh.C, sh.T,
                       (int)(b->s0 % (uint64_t)M), d_out);
    FSEA_HIP(hipGetLastError());
    b->state.advance();
    b->s0 += n;
    if (F) {
        rc = fsea_detail::launch(b->plan, fsea::IN_F32, d_out, F, 0, b->mode, d_rows, s);
        if (rc) return rc;
    }
    if (d_series && F) {
        const dim3 tgrid((unsigned)((M + PF_TR - 1) / PF_TR), (unsigned)((F + PF_TR - 1) / PF_TR));
        hipLaunchKernelGGL(fsea_pfb_transpose, tgrid, dim3(PF_WG), 0, s, (const cf *)d_rows, (long long)F, M,
                           static_cast<cf *>(d_series));
        FSEA_HIP(hipGetLastError());
    }
    if (d_frames && F) FSEA_HIP(hipMemcpyAsync(d_frames, d_out, n_out * sizeof(cf), hipMemcpyDeviceToDevice, s));
    return b->frames.release(s);
}

}  // namespace

extern "C" {

int fsea_pfb_prototype(int channels, int branch_taps, double *taps) {
    if (!taps) return fail(FSEA_EINVAL, "taps is NULL");
    if (int rc = check_shape(channels, branch_taps)) return rc;
    const int L = channels * branch_taps;
    if (int rc = fsea_fir_lowpass_taps(2.0 * channels, 1.0, L, taps)) return rc;
    for (int j = 0; j < L; ++j) taps[j] = (double)channels * taps[j];
    return FSEA_OK;
}

int fsea_pfb_create(fsea_pfb **out, const double *taps, int channels, int branch_taps, int oversampling, int mode, int device) {
    if (!out) return fail(FSEA_EINVAL, "pfb out-pointer is NULL");
    *out = nullptr;
    if (!taps) return fail(FSEA_EINVAL, "taps is NULL");
    if (int rc = check_shape(channels, branch_taps)) return rc;
    if ((oversampling != 1 && oversampling != 2 && oversampling != 4) || channels % oversampling) {
        return fail(FSEA_EINVAL, "oversampling must be 1, 2 or 4 and divide the %d channels, got %d", channels, oversampling);
    }
    const int L = channels * branch_taps;
    if (int rc = FirState::check_finite(taps, L)) return rc;
    return fsea_detail::create_object(out, device, "fsea_pfb_create", [&](fsea_pfb *b) -> int {
        b->channels = channels;
        b->branch_taps = branch_taps;
        b->oversampling = oversampling;
        b->mode = mode;
        int rc = fsea_plan_create(&b->plan.ptr, channels, channels, mode, device);   // the modes of any plan, and its statuses
        if (rc) return rc;
        hipError_t e = b->state.create(taps, L, L, (size_t)L - 1);
        if (e == hipSuccess) e = b->frames.create(b->staging.stream);
        return fsea_detail::init_code("fsea_pfb_create", e);
    });
}

int fsea_pfb_destroy(fsea_pfb *b) { return fsea_detail::destroy_object(b); }

int fsea_pfb_reset(fsea_pfb *b) {
    return fsea_detail::reset_object(b, "pfb is NULL", [&] {
        b->s0 = 0;
        return b->state.reset();
    });
}

size_t fsea_pfb_out_frames(const fsea_pfb *b, size_t n_samples) { return b ? out_frames(b, n_samples) : 0; }

size_t fsea_pfb_row_bytes(const fsea_pfb *b) { return b ? fsea_plan_row_bytes(b->plan) : 0; }

int fsea_pfb_run_device(fsea_pfb *b, const void *d_iq, size_t n_samples, int flip, void *d_rows, void *d_frames, void *d_series,
                        void *stream) {
    int rc = check_run(b, d_iq, n_samples, d_series);
    if (!rc) rc = fsea_detail::check_aligned16("d_iq, d_rows, d_frames and d_series", d_iq, d_rows, d_frames);
    if (!rc) rc = fsea_detail::check_aligned16("d_iq, d_rows, d_frames and d_series", d_series);
    if (!rc) rc = check_outputs(b, n_samples, d_rows);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(b->mu);
    FSEA_ON_DEVICE(b->device);
    return queue_call(b, d_iq, n_samples, flip, d_rows, d_frames, d_series, static_cast<hipStream_t>(stream));
}

int fsea_pfb_run_host(fsea_pfb *b, const uint8_t *iq, size_t n_samples, int flip, void *rows, float *frames, float *series) {
    int rc = check_run(b, iq, n_samples, series);
    if (!rc) rc = check_outputs(b, n_samples, rows);
    if (rc) return rc;
    if (n_samples == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(b->mu);
    FSEA_ON_DEVICE(b->device);
    const size_t F = out_frames(b, n_samples), pairs_bytes = F * (size_t)b->channels * sizeof(cf);
    const fsea_detail::HostStaging::Part parts[3] = {{rows, F * fsea_plan_row_bytes(b->plan)}, {frames, pairs_bytes},
                                                     {series, pairs_bytes}};
    return b->staging.run(
        2 * n_samples, parts, [&](void *h_in) { std::memcpy(h_in, iq, 2 * n_samples); },
        [&](void *d_in, void **d_parts, hipStream_t s) {
            return queue_call(b, d_in, n_samples, flip, d_parts[0], d_parts[1], d_parts[2], s);
        });
}

}  // extern "C"
