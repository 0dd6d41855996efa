// fsea_zoom_image.h -- what the two decimating kernels share: fsea_shift_decim_u8 (fsea_zoom.hip: one stream, a tail from
// call to call) and fsea_extract_u8 (fsea_extract.hip: a table of jobs over one resident recording).  Both stage a tile's
// rotated samples phase-major in LDS and run one FMA chain per output over it; the geometry of that image, its three
// capacities, the byte-offset table of the taps' samples, the store loop and the chain are here, so that a job of the one is
// a freshly reset call of the other, bit for bit.  How a sample is loaded and rotated is fsea_fir_stage.h's.
#pragma once

#include "fsea_fir_stage.h"

namespace fsea_zoom_image {

using namespace fsea_stage;

constexpr int ZM_WG = 256;                       // lanes per workgroup: all of them stage
constexpr int ZM_T = FSEA_ZOOM_TILE_OUTPUTS;     // outputs per workgroup, one per lane of the first two waves
constexpr int ZM_TAPS_ALLOC = FSEA_FIR_MAX_TAPS + 8;   // padded taps on the device (zeros past L): whole groups of eight
constexpr int ZM_CAP_S = 2304, ZM_CAP_M = 4608, ZM_CAP_L = 8832;   // samples of the three LDS images
constexpr size_t ZM_MAX_SAMPLES = (size_t)1 << 31;
static_assert(ZM_T <= ZM_WG && ZM_T % 64 == 0, "whole waves own the outputs, one per lane");

// columns of the phase-major image: sample m of the tile at [m % D][m / D], m < ZM_T D + L - 1; odd
constexpr int zoom_pitch(int D, int L) { return (ZM_T + (L - 1 + D - 1) / D) | 1; }
constexpr int zoom_lds_samples(int D, int L) { return D * zoom_pitch(D, L); }
static_assert(zoom_lds_samples(FSEA_ZOOM_MAX_DECIMATION, FSEA_FIR_MAX_TAPS) <= ZM_CAP_L, "the largest image fits");
static_assert(2 * ZM_CAP_L * sizeof(cf) <= 160 * 1024, "two workgroups per CU at the largest L and D");

// the byte offsets of the taps' samples in the image, from a lane's column: tap k reads [k % D][k / D]; 0 past n_taps
inline void zoom_fill_offsets(uint32_t offs[ZM_TAPS_ALLOC], int n_taps, int decimation) {
    for (int k = 0; k < ZM_TAPS_ALLOC; ++k) offs[k] = 0;
    for (int k = 0; k < n_taps; ++k) {
        offs[k] = (uint32_t)(((k % decimation) * zoom_pitch(decimation, n_taps) + k / decimation) * (int)sizeof(cf));
    }
}

// One staged group into the image: v[j] is the tile's sample m0 + j (m0 negative in a tile's first group only); the samples
// below 0 and from `span` on are not the tile's.
__device__ __forceinline__ void zoom_store_group(cf *lds, const cf v[8], int m0, int span, int D, int pitch) {
    int q = m0 > 0 ? m0 / D : 0, r = m0 > 0 ? m0 - q * D : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int m = m0 + j;
        if (m >= 0) {
            if (m < span) lds[r * pitch + q] = v[j];
            if (++r == D) {
                r = 0;
                ++q;
            }
        }
    }
}

// One output: one FMA chain over the taps ascending, from +0.  col = the image at the lane's column: sample i D + k stands
// at [k % D][i + k / D], the same byte offset from col for every lane.  Those offsets are a table in device memory (made
// once per object: D and L are its constants), read like the taps by scalar loads -- stepping k % D and k / D in the loop
// instead cost eight scalar instructions per tap, more than the CU's one scalar unit has time for at small D.  Eight taps
// at a time; past L the table holds offset 0 (a staged, finite sample) for the zero taps behind the filter's own.
__device__ __forceinline__ cf zoom_chain(const cf *col, const float *__restrict__ taps, const uint32_t *__restrict__ offs, int L) {
    const cf *taps2 = reinterpret_cast<const cf *>(taps);   // tap pairs, one SGPR pair each
    const char *base = reinterpret_cast<const char *>(col);
    cf acc = cf{0.0f, 0.0f};
    for (int k0 = 0; k0 < L; k0 += 8) {
        cf x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const cf *>(base + offs[k0 + j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const cf t = taps2[(k0 >> 1) + j];
            acc = pk_tap_fma_lo(x[2 * j], t, acc);
            acc = pk_tap_fma_hi(x[2 * j + 1], t, acc);
        }
    }
    return acc;
}

}  // namespace fsea_zoom_image
