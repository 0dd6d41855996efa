// fsea_zoom.hip -- the zoom spectrum (include/fsea.h: fsea_zoom_*): frequency shift -> low-pass -> keep every D-th sample ->
// FFT, the chain the reference runs inside nrf_decoder (nrf_freq_shifter, nrf_downsampler, nrf_fft) offered as a spectrum.
// A call reads the 8-bit stream once and leaves n / D filtered pairs resident for the object's own fsea_plan.
//
// Kernel fsea_shift_decim_u8 ("The zoom spectrum"): output i of a call is
//   pairs[i] = sum_{k < L} c[k] x_ext[i D + k],   x_ext = tail ++ x,   i < n / D,
// x the rotated samples of fsea_shift_fir_u8 (fsea_fir_stage.h: the same helpers, so the same bits), one accumulator per
// output, taps ascending -- output i is output i D of the full-rate filter, bit for bit.  One workgroup of ZM_WG = 256 lanes
// per tile of ZM_T = 128 outputs.  All four waves stage the tile's ZM_T D + L - 1 rotated samples once in LDS (the rotation,
// some twenty VALU operations per input sample, is most of the work from D = 8 or so on), then the first two run one
// output per lane.  The image is phase-major: sample m of the tile at [m mod D][m / D], so that the 64 lanes of a wave, which read samples i D + k for
// consecutive i, read consecutive 8-byte words (k mod D and k / D are the same for every lane).  The row pitch is odd, so
// the staging stores of neighbouring phases fall on different banks.  Taps arrive by scalar loads and are broadcast into
// v_pk_fma_f32 as in the filter, and so do the byte offsets of the taps' samples in the image (a table per object); the outputs are 8-byte stores, 512 contiguous bytes per wave.  The LDS image is a static
// array in three sizes (18, 36 and 69 KiB: kernels ..._s, ..._m and the plain name), the launch picks the smallest that
// holds D (ZM_T + ceil((L - 1) / D)) samples: eight, four and two workgroups per CU.  A tile of 128 outputs keeps two
// workgroups on a CU at D = 64, L = 512; a lane with several outputs would need an image several times that.  Workgroup 0 writes the next tail into
// the second of two tail buffers, as the filter does.
#include "fsea_zoom_image.h"

#include <cmath>

using fsea_detail::DeviceGuard;
using fsea_detail::fail;
using namespace fsea_zoom_image;   // the image, the chain and fsea_stage

namespace {

template <int CAP>
__device__ __forceinline__ void zoom_body(const void *__restrict__ in, long long n, uint32_t flip, const cf *__restrict__ tail_in,
                                          cf *__restrict__ tail_out, const float *__restrict__ taps,
                                          const uint32_t *__restrict__ offs, int L, int D, cf *__restrict__ out,
                                          const FirRot &rot) {
    __shared__ __attribute__((aligned(16))) cf lds[CAP];
    const int tid = threadIdx.x;
    const int pitch = zoom_pitch(D, L);
    const long long n_out = n / D;
    const long long i0 = (long long)blockIdx.x * ZM_T;             // first output of the tile
    const long long left = n_out - i0;                             // outputs from there on (0: a call with no output)
    const int n_tile = left < ZM_T ? (int)left : ZM_T;
    const int span = n_tile > 0 ? n_tile * D + L - 1 : 0;          // x_ext entries the tile reads, from i0 D
    const long long s_first = i0 * D - (L - 1);                    // input sample of x_ext[i0 D] (negative: the tail)
    const long long s_al = s_first & ~7LL;                         // the 8-sample group it lies in
    const int groups = span ? (int)((s_first - s_al + span + 7) >> 3) : 0;

    // stage: x_ext[i0 D + m], m < span, rotated, phase-major.  Every entry a stored output reads lies inside the input or
    // the tail: (n_out - 1) D + L - 1 < n + L - 1.
    for (int g = tid; g < groups; g += ZM_WG) {
        const long long s = s_al + 8LL * g;
        cf v[8];
        stage_group<FIR_IN_U8, true>(in, s, n, flip, tail_in, L, rot, v);
        const int m0 = (int)(s - s_first);      // tile position of the group's sample 0; negative in the first group only
        zoom_store_group(lds, v, m0, span, D, pitch);
    }
    __syncthreads();

    // the first two waves: lane i's output
    if (tid < ZM_T) {
        const cf acc = zoom_chain(lds + tid, taps, offs, L);
        if (tid < n_tile) out[i0 + tid] = acc;
    }

    // the next call's tail: x_ext[n + m], m < L - 1 -- from the old tail while n + m < L - 1 (a call shorter than the tail)
    if (blockIdx.x == 0) {
        for (int m = tid; m < L - 1; m += ZM_WG) {
            const long long e = n + m;
            tail_out[m] = e < L - 1 ? tail_in[e] : load_input<FIR_IN_U8, true>(in, e - (L - 1), flip, rot);
        }
    }
}

}  // namespace

#define FSEA_ZOOM_KERNEL(name, cap)                                                                                       \
    extern "C" __global__ __launch_bounds__(ZM_WG) void name(                                                             \
        const void *__restrict__ in, long long n, uint32_t flip, const cf *__restrict__ tail_in, cf *__restrict__ tail_out, \
        const float *__restrict__ taps, const uint32_t *__restrict__ offs, int L, int D, cf *__restrict__ out, FirRot rot) { \
        zoom_body<cap>(in, n, flip, tail_in, tail_out, taps, offs, L, D, out, rot);                                       \
    }
FSEA_ZOOM_KERNEL(fsea_shift_decim_u8_s, ZM_CAP_S)
FSEA_ZOOM_KERNEL(fsea_shift_decim_u8_m, ZM_CAP_M)
FSEA_ZOOM_KERNEL(fsea_shift_decim_u8, ZM_CAP_L)

struct fsea_zoom {
    int n_taps = 0;
    int decimation = 1;
    int device = 0;
    FirState state;                               // ZM_TAPS_ALLOC floats of taps, the two tails
    fsea_detail::DeviceArray<uint32_t> d_offs;    // ZM_TAPS_ALLOC byte offsets of the taps' samples in the LDS image, 0 past n_taps
    fsea_detail::SharedScratch pairs;             // the decimated pairs of the last call; its event orders the calls
    std::mutex mu;
    fsea_detail::HostStaging staging;             // the host form
    fsea_detail::Owned<fsea_plan, fsea_plan_destroy> plan;   // (fft_size, hop, mode) on the decimated pairs; the first to go
};

namespace {

size_t out_rows(const fsea_zoom *z, size_t n_samples) {
    const size_t n_out = n_samples / (size_t)z->decimation, N = (size_t)z->plan->n;
    return n_out >= N ? (n_out - N) / (size_t)z->plan->hop + 1 : 0;
}

// what a run checks before it looks into the object
int check_run(const fsea_zoom *z, const void *iq, size_t n, double cycles_per_sample, double phase0_cycles, uint64_t offset) {
    if (!z) return fail(FSEA_EINVAL, "zoom is NULL");
    if (n > ZM_MAX_SAMPLES) return fail(FSEA_EINVAL, "n_samples %zu too large", n);
    if (int rc = check_shift(cycles_per_sample, phase0_cycles, offset, n)) return rc;
    if (n && !iq) return fail(FSEA_EINVAL, "NULL buffer");
    return FSEA_OK;
}

int check_rows(const fsea_zoom *z, size_t n, const void *rows) {
    return out_rows(z, n) && !rows ? fail(FSEA_EINVAL, "NULL buffer for the %zu rows of the call", out_rows(z, n)) : (int)FSEA_OK;
}

// One call on device buffers, asynchronous on `s`: the decimating launch into the object's pairs, the plan's launch on
// them, the copy of the pairs where asked for.  The caller holds z->mu and is on z's device.
int queue_call(fsea_zoom *z, const void *d_iq, size_t n, int flip, const FirRot &rot, void *d_rows, void *d_pairs, hipStream_t s) {
    const int D = z->decimation, L = z->n_taps;
    const size_t n_out = n / (size_t)D, rows = out_rows(z, n);
    if (n == 0) return FSEA_OK;
    // every call, on whatever stream, follows the previous user of the pairs and the tails
    int rc = z->pairs.acquire(n_out * sizeof(cf) + 16, s);
    if (rc) return rc;
    cf *d_out = static_cast<cf *>(z->pairs.buf.ptr);
    const unsigned grid = n_out ? (unsigned)((n_out + ZM_T - 1) / ZM_T) : 1u;   // no output: the tail still advances
    const int need = zoom_lds_samples(D, L);
    auto kernel = need <= ZM_CAP_S ? fsea_shift_decim_u8_s : need <= ZM_CAP_M ? fsea_shift_decim_u8_m : fsea_shift_decim_u8;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(ZM_WG), 0, s, d_iq, (long long)n, flip ? 0x80808080u : 0u,
                       z->state.in(), z->state.out(), (const float *)z->state.taps.ptr, (const uint32_t *)z->d_offs.ptr, L, D,
                       d_out, rot);
    FSEA_HIP(hipGetLastError());
    z->state.advance();
    if (rows) {
        rc = fsea_detail::launch(z->plan, fsea::IN_F32, d_out, rows, 0, z->plan->mode, d_rows, s);
        if (rc) return rc;
    }
    if (d_pairs && n_out) FSEA_HIP(hipMemcpyAsync(d_pairs, d_out, n_out * sizeof(cf), hipMemcpyDeviceToDevice, s));
    return z->pairs.release(s);
}

}  // namespace

extern "C" {

int fsea_zoom_create(fsea_zoom **out, const double *taps, int n_taps, int decimation, int fft_size, int hop, int mode,
                     int device) {
    if (!out) return fail(FSEA_EINVAL, "zoom out-pointer is NULL");
    *out = nullptr;
    if (int rc = FirState::check_taps(taps, n_taps)) return rc;
    if (decimation < 1 || decimation > FSEA_ZOOM_MAX_DECIMATION) {
        return fail(FSEA_EINVAL, "decimation must be in [1, %d], got %d", FSEA_ZOOM_MAX_DECIMATION, decimation);
    }
    return fsea_detail::create_object(out, device, "fsea_zoom_create", [&](fsea_zoom *z) -> int {
        z->n_taps = n_taps;
        z->decimation = decimation;
        int rc = fsea_plan_create(&z->plan.ptr, fft_size, hop, mode, device);   // the sizes and modes of any plan, and its statuses
        if (rc) return rc;
        uint32_t offs[ZM_TAPS_ALLOC];
        zoom_fill_offsets(offs, n_taps, decimation);
        hipError_t e = z->state.create(taps, n_taps, ZM_TAPS_ALLOC, FSEA_FIR_MAX_TAPS);
        if (e == hipSuccess) e = z->d_offs.upload(offs, ZM_TAPS_ALLOC);
        if (e == hipSuccess) e = z->pairs.create(z->staging.stream);
        return fsea_detail::init_code("fsea_zoom_create", e);
    });
}

int fsea_zoom_destroy(fsea_zoom *z) { return fsea_detail::destroy_object(z); }

int fsea_zoom_reset(fsea_zoom *z) {
    return fsea_detail::reset_object(z, "zoom is NULL", [&] { return z->state.reset(); });
}

int fsea_zoom_set_window(fsea_zoom *z, const float *w) {
    if (!z) return fail(FSEA_EINVAL, "zoom is NULL");
    std::lock_guard<std::mutex> lock(z->mu);
    return fsea_plan_set_window(z->plan, w);
}

size_t fsea_zoom_out_pairs(const fsea_zoom *z, size_t n_samples) { return z ? n_samples / (size_t)z->decimation : 0; }

size_t fsea_zoom_out_rows(const fsea_zoom *z, size_t n_samples) { return z ? out_rows(z, n_samples) : 0; }

size_t fsea_zoom_row_bytes(const fsea_zoom *z) { return z ? fsea_plan_row_bytes(z->plan) : 0; }

int fsea_zoom_run_device(fsea_zoom *z, const void *d_iq, size_t n_samples, int flip, double cycles_per_sample,
                         double phase0_cycles, uint64_t sample_offset, void *d_rows, void *d_pairs, void *stream) {
    int rc = check_run(z, d_iq, n_samples, cycles_per_sample, phase0_cycles, sample_offset);
    if (!rc) rc = fsea_detail::check_aligned16("d_iq, d_rows and d_pairs", d_iq, d_rows, d_pairs);
    if (!rc) rc = check_rows(z, n_samples, d_rows);
    if (rc) return rc;
    const FirRot rot = make_rot(cycles_per_sample, phase0_cycles, sample_offset, n_samples);
    std::lock_guard<std::mutex> lock(z->mu);
    FSEA_ON_DEVICE(z->device);
    return queue_call(z, d_iq, n_samples, flip, rot, d_rows, d_pairs, static_cast<hipStream_t>(stream));
}

int fsea_zoom_run_host(fsea_zoom *z, const uint8_t *iq, size_t n_samples, int flip, double cycles_per_sample,
                       double phase0_cycles, uint64_t sample_offset, void *rows, float *pairs) {
    int rc = check_run(z, iq, n_samples, cycles_per_sample, phase0_cycles, sample_offset);
    if (!rc) rc = check_rows(z, n_samples, rows);
    if (rc) return rc;
    if (n_samples == 0) return FSEA_OK;
    const FirRot rot = make_rot(cycles_per_sample, phase0_cycles, sample_offset, n_samples);
    std::lock_guard<std::mutex> lock(z->mu);
    FSEA_ON_DEVICE(z->device);
    const fsea_detail::HostStaging::Part parts[2] = {{rows, out_rows(z, n_samples) * fsea_plan_row_bytes(z->plan)},
                                                     {pairs, n_samples / (size_t)z->decimation * sizeof(cf)}};
    return z->staging.run(
        2 * n_samples, parts, [&](void *h_in) { std::memcpy(h_in, iq, 2 * n_samples); },
        [&](void *d_in, void **d_parts, hipStream_t s) { return queue_call(z, d_in, n_samples, flip, rot, d_parts[0], d_parts[1], s); });
}

}  // extern "C"
