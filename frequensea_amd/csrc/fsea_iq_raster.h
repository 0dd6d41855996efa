// fsea_iq_raster.h -- the line rasteriser that fsea_iq_draw.hip (fsea_iq_lines_*) and fsea_trace.hip (fsea_trace_hits_*)
// share: pixel t of the reference's draw_line in closed form, and the wave-wide deal of a wave's pixels to its lanes.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace fsea_detail {

// Pixel t (0 <= t <= max(dx, dy)) of the reference's draw_line from (x1, y1) to (x2, y2), dx = |x2 - x1|, dy = |y2 - y1|:
// with err0 = (dx > dy ? dx : -dy) / 2 the major axis (x if dx > dy, else y) moves at every step, and the minor
// coordinate after t steps is the unique integer k with 0 <= h - t*d + L*k < L (L the major, d the minor delta,
// h = L / 2), i.e. k = (t*d - h + L - 1) / L.  A and B hold the endpoints as x | y << 16.
__device__ __forceinline__ void line_xy(uint32_t A, uint32_t B, uint32_t t, int &x, int &y) {
    const int x1 = (int)(A & 0xffffu), y1 = (int)(A >> 16), x2 = (int)(B & 0xffffu), y2 = (int)(B >> 16);
    const int dx = abs(x2 - x1), dy = abs(y2 - y1);
    const int sx = x1 < x2 ? 1 : -1, sy = y1 < y2 ? 1 : -1;
    const bool xmajor = dx > dy;
    const uint32_t L = (uint32_t)(xmajor ? dx : dy), d = (uint32_t)(xmajor ? dy : dx);
    const uint32_t k = L ? (t * d - L / 2 + L - 1) / L : 0u;
    x = x1 + sx * (int)(xmajor ? t : k);
    y = y1 + sy * (int)(xmajor ? k : t);
}

__device__ __forceinline__ uint32_t line_pixel(uint32_t A, uint32_t B, uint32_t t, uint32_t stride) {
    int x, y;
    line_xy(A, B, t, x, y);
    return (uint32_t)y * stride + (uint32_t)x;
}

// The segments of one wave, one per lane (endpoints A and B, len = max(dx, dy) + 1 pixels, 0 for a lane without a
// segment): an inclusive prefix sum of the pixel counts across the wave, then the wave's pixels 64 at a time, so that a long
// segment is drawn by many lanes.  plot(A, B, t) is called once for every pixel t of every segment.  Every lane of the wave
// must call this (the shuffles read other lanes' registers); only plot is predicated.
template <class Plot>
__device__ __forceinline__ void wave_lines(uint32_t A, uint32_t B, uint32_t len, int lane, Plot &&plot) {
    uint32_t incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    for (uint32_t base = 0; base < total; base += 64) {
        const uint32_t p = base + lane;
        // the lane whose segment holds pixel p: the first with incl > p
        int lo = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
            if (__shfl(incl, lo + step - 1, 64) <= p) lo += step;
        }
        const uint32_t sA = __shfl(A, lo, 64), sB = __shfl(B, lo, 64);
        const uint32_t start = __shfl(incl, lo, 64) - __shfl(len, lo, 64);
        if (p < total) plot(sA, sB, p - start);
    }
}

}  // namespace fsea_detail
