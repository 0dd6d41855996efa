// fsea_trace.hip -- the IQ trace movie (include/fsea.h: fsea_trace_*): the frame loop of the reference's c/single-sample.c
// (its lines 126-149) on a canvas that lives on the device.
//
// A frame fades the whole canvas, then draws the frame's segments with the tool's pixel_inc: a hit on a pixel of value v
// adds pixel_inc unless v + pixel_inc >= 255.  All hits of one frame on one pixel are that same operation, so h hits on a
// faded value v leave v + p min(h, (254 - v) / p): a frame is per-pixel hit counts followed by a per-pixel recurrence over
// the frames ("The IQ trace movie").  A launch works on a chunk of frames in two passes:
//
// Hit pass (fsea_trace_hits_b8 / _b32): the rasteriser of fsea_iq_lines_* (fsea_iq_raster.h), one lane per segment, the
// wave's pixels dealt out 64 at a time, counting into one plane of (256 m)^2 counts per frame.  The planes cover the IQ
// square only.  A segment hits a pixel at most once, so while a frame has at most 255 segments a count fits a byte: four
// counts share a u32 and a hit adds 1 << 8 (x & 3) to it (_b8).  Longer frames count in u32 (_b32).
//
// Compose pass (fsea_trace_compose_*): a lane owns 16 consecutive canvas bytes and keeps them in registers across the
// chunk's frames.  Per frame it fades them, adds the hits where its bytes meet the IQ square, and writes one 16-byte store
// into that frame's image; after the last frame it writes the bytes back to the canvas.  The counts of TR_BATCH frames are
// loaded ahead of their use.  Outside the IQ square the canvas is zero for ever: such a lane loads nothing.  All workgroups
// walk the chunk's frames in the same order, so those in flight at one time write neighbouring pieces of the same few
// frames ("Placement").  The plain kernels need a width and a left margin of the IQ square that are multiples
// of 16: a lane's bytes then lie in one row, wholly inside or outside the square, and their counts are one aligned load.
// The _any kernels take every other geometry: each byte finds its own count, and a frame that does not start at a
// multiple of 16 bytes is written byte by byte.
#include "fsea_internal.h"
#include "fsea_iq_raster.h"

#include <algorithm>
#include <cstring>

using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int IQ_RES = 256;
constexpr int TR_WG = 256;
constexpr int TR_BATCH = 4;                              // frames whose counts a compose lane has in flight
constexpr int TR_MAX_SIDE = 16384;                       // canvas width and height at most
constexpr int TR_MAX_CHUNK = 4096;                       // frames per pair of launches at most
constexpr size_t TR_COUNT_BYTES = (size_t)64 << 20;      // count planes of one chunk
constexpr size_t TR_MAX_FRAME_BYTES = (size_t)1 << 31;
constexpr size_t TR_MAX_OUT = (size_t)1 << 40;

struct TraceGeo {
    int width, height;  // of the canvas
    int side;           // of the IQ square, 256 m
    int m;
    int ox, oy;         // where the IQ square starts in the canvas
    int inc, fade;
    uint32_t magic;     // ceil(2^16 / inc): (n * magic) >> 16 == n / inc for 0 <= n <= 254
};

// grid (ceil(segments / TR_WG), frames of this launch); frame f of the launch starts at byte f * frame_bytes; counts: one
// plane of side^2 counts of CB bytes per frame
template <int CB>
__device__ __forceinline__ void hits_body(const uint8_t *__restrict__ bytes, long long n_bytes, long long frame_bytes,
                                          uint32_t flip, TraceGeo g, uint32_t *__restrict__ counts) {
    const long long j = (long long)blockIdx.y * frame_bytes;
    // the frame's points: 2 k < frame_bytes, and both bytes of the point inside the data
    long long np = (frame_bytes + 1) / 2;
    const long long avail = n_bytes > j ? (n_bytes - j) / 2 : 0;
    if (avail < np) np = avail;
    uint32_t *plane = counts + (size_t)blockIdx.y * ((size_t)g.side * g.side * CB / 4);
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * TR_WG + threadIdx.x;  // segment s: point s to point s + 1

    uint32_t A = 0u, B = 0u, len = 0u;
    if (s + 1 < np) {
        const uint8_t *p = bytes + j + 2 * s;
        const uint32_t I1 = p[0] ^ flip, Q1 = p[1] ^ flip, I2 = p[2] ^ flip, Q2 = p[3] ^ flip;
        A = I1 * g.m | (Q1 * g.m) << 16;
        B = I2 * g.m | (Q2 * g.m) << 16;
        const int dx = abs((int)(I2 - I1)) * g.m, dy = abs((int)(Q2 - Q1)) * g.m;
        len = (uint32_t)max(dx, dy) + 1u;
    }
    fsea_detail::wave_lines(A, B, len, lane, [&](uint32_t sA, uint32_t sB, uint32_t t) {
        int x, y;
        fsea_detail::line_xy(sA, sB, t, x, y);
        // the tool's pixel_inc compares IQ-square coordinates with the canvas size
        if (x == 0 || y == 0 || x == g.width - 1 || y == g.height - 1) return;
        const uint32_t px = (uint32_t)y * (uint32_t)g.side + (uint32_t)x;
        if (CB == 1) atomicAdd(plane + (px >> 2), 1u << (8 * (px & 3u)));
        else atomicAdd(plane + px, 1u);
    });
}

// the counts of 16 consecutive pixels from px on (a multiple of 16), as bytes, counts above 255 as 255
template <int CB>
__device__ __forceinline__ uint4 load_hits(const uint8_t *__restrict__ plane, uint32_t px) {
    if (CB == 1) return *reinterpret_cast<const uint4 *>(plane + px);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 c = reinterpret_cast<const uint4 *>(plane)[px / 4 + k];
        w[k] = min(c.x, 255u) | min(c.y, 255u) << 8 | min(c.z, 255u) << 16 | min(c.w, 255u) << 24;
    }
    return uint4{w[0], w[1], w[2], w[3]};
}

// the same for 16 pixels that each have an offset of their own (negative: outside the IQ square)
template <int CB>
__device__ __forceinline__ uint4 gather_hits(const uint8_t *__restrict__ plane, const int *off) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        uint32_t c = 0u;
        if (off[k] >= 0) c = CB == 1 ? (uint32_t)plane[off[k]] : min(reinterpret_cast<const uint32_t *>(plane)[off[k]], 255u);
        w[k >> 2] |= c << (8 * (k & 3));
    }
    return uint4{w[0], w[1], w[2], w[3]};
}

// one frame on four canvas bytes: fade, then h hits per byte
__device__ __forceinline__ uint32_t frame_word(uint32_t v, uint32_t h, const TraceGeo &g) {
    if ((g.fade == 0 || v == 0u) && h == 0u) return v;
    uint32_t out = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t b = (v >> (8 * k)) & 0xffu;
        const uint32_t hb = (h >> (8 * k)) & 0xffu;
        b = b > (uint32_t)g.fade ? b - (uint32_t)g.fade : 0u;
        b += (uint32_t)g.inc * min(hb, ((254u - b) * g.magic) >> 16);
        out |= b << (8 * k);
    }
    return out;
}

// grid (ceil(groups of 16 canvas bytes / TR_WG)); counts: n_frames planes; canvas: padded to whole groups;
// images: n_frames images, or null (the canvas advances, no frame is written)
template <int CB, bool ALIGNED>
__device__ __forceinline__ void compose_body(const uint8_t *__restrict__ counts, int n_frames, TraceGeo g,
                                             uint8_t *__restrict__ canvas, uint8_t *__restrict__ images) {
    const uint32_t WH = (uint32_t)g.width * (uint32_t)g.height;  // at most 2^28
    const uint32_t group = blockIdx.x * TR_WG + threadIdx.x;
    if (group >= (WH + 15u) / 16u) return;
    const uint32_t c0 = 16u * group;
    const size_t plane = (size_t)g.side * g.side * CB;

    bool inside = false;
    uint32_t px0 = 0u;
    int off[ALIGNED ? 1 : 16];
    if (ALIGNED) {
        const int y = (int)(c0 / (uint32_t)g.width), x = (int)(c0 - (uint32_t)y * (uint32_t)g.width);
        inside = x >= g.ox && x < g.ox + g.side && y >= g.oy && y < g.oy + g.side;
        px0 = inside ? (uint32_t)(y - g.oy) * (uint32_t)g.side + (uint32_t)(x - g.ox) : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t c = c0 + k;
            const int y = (int)(c / (uint32_t)g.width), x = (int)(c - (uint32_t)y * (uint32_t)g.width);
            const bool ok = c < WH && x >= g.ox && x < g.ox + g.side && y >= g.oy && y < g.oy + g.side;
            off[k] = ok ? (y - g.oy) * g.side + (x - g.ox) : -1;
            inside = inside || ok;
        }
    }
    if (!inside && images == nullptr) return;

    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (inside) v = *reinterpret_cast<const uint4 *>(canvas + c0);
    constexpr int BATCH = ALIGNED ? TR_BATCH : 1;  // the gathers of one frame are 16 loads already
    for (int f0 = 0; f0 < n_frames; f0 += BATCH) {
        uint4 h[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            h[b] = uint4{0u, 0u, 0u, 0u};
            if (inside && f0 + b < n_frames) {
                const uint8_t *pl = counts + (size_t)(f0 + b) * plane;
                h[b] = ALIGNED ? load_hits<CB>(pl, px0) : gather_hits<CB>(pl, off);
            }
        }
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            if (f0 + b >= n_frames) break;
            if (inside) {
                v.x = frame_word(v.x, h[b].x, g);
                v.y = frame_word(v.y, h[b].y, g);
                v.z = frame_word(v.z, h[b].z, g);
                v.w = frame_word(v.w, h[b].w, g);
            }
            if (images == nullptr) continue;
            uint8_t *dst = images + (size_t)(f0 + b) * WH + c0;
            if (ALIGNED || ((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && c0 + 16u <= WH)) {
                *reinterpret_cast<uint4 *>(dst) = v;
            } else {
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if (c0 + k < WH) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
    }
    if (inside) *reinterpret_cast<uint4 *>(canvas + c0) = v;
}

}  // namespace

extern "C" __global__ __launch_bounds__(TR_WG) void fsea_trace_hits_b8(const uint8_t *__restrict__ bytes, long long n_bytes,
                                                                       long long frame_bytes, uint32_t flip, TraceGeo g,
                                                                       uint32_t *__restrict__ counts) {
    hits_body<1>(bytes, n_bytes, frame_bytes, flip, g, counts);
}
extern "C" __global__ __launch_bounds__(TR_WG) void fsea_trace_hits_b32(const uint8_t *__restrict__ bytes, long long n_bytes,
                                                                        long long frame_bytes, uint32_t flip, TraceGeo g,
                                                                        uint32_t *__restrict__ counts) {
    hits_body<4>(bytes, n_bytes, frame_bytes, flip, g, counts);
}

extern "C" __global__ __launch_bounds__(TR_WG) void fsea_trace_compose_b8(const uint8_t *__restrict__ counts, int n_frames,
                                                                          TraceGeo g, uint8_t *__restrict__ canvas,
                                                                          uint8_t *__restrict__ images) {
    compose_body<1, true>(counts, n_frames, g, canvas, images);
}
extern "C" __global__ __launch_bounds__(TR_WG) void fsea_trace_compose_b32(const uint8_t *__restrict__ counts, int n_frames,
                                                                           TraceGeo g, uint8_t *__restrict__ canvas,
                                                                           uint8_t *__restrict__ images) {
    compose_body<4, true>(counts, n_frames, g, canvas, images);
}
extern "C" __global__ __launch_bounds__(TR_WG) void fsea_trace_compose_b8_any(const uint8_t *__restrict__ counts,
                                                                              int n_frames, TraceGeo g,
                                                                              uint8_t *__restrict__ canvas,
                                                                              uint8_t *__restrict__ images) {
    compose_body<1, false>(counts, n_frames, g, canvas, images);
}
extern "C" __global__ __launch_bounds__(TR_WG) void fsea_trace_compose_b32_any(const uint8_t *__restrict__ counts,
                                                                               int n_frames, TraceGeo g,
                                                                               uint8_t *__restrict__ canvas,
                                                                               uint8_t *__restrict__ images) {
    compose_body<4, false>(counts, n_frames, g, canvas, images);
}

struct fsea_trace {
    int device = 0;
    TraceGeo g = {};
    std::mutex mu;
    fsea_detail::DeviceArray<uint8_t> canvas;  // width x height bytes, padded to a whole 16-byte group
    size_t canvas_bytes = 0;
    fsea_detail::SharedScratch counts;  // the count planes of one chunk; its event orders the uses of the canvas too
    fsea_detail::HostStaging staging;   // the host-buffer forms
};

namespace {

size_t frame_pixels(const fsea_trace *t) { return (size_t)t->g.width * t->g.height; }

// what does not look at the object comes first: a test can pass an object that is never dereferenced
int check_frames(const fsea_trace *t, const void *bytes, size_t n_bytes, size_t frame_bytes, int n_frames) {
    if (!t) return fail(FSEA_EINVAL, "trace is NULL");
    if (frame_bytes == 0 || frame_bytes > TR_MAX_FRAME_BYTES) {
        return fail(FSEA_EINVAL, "frame_bytes must be in [1, 2^31], got %zu", frame_bytes);
    }
    if (int rc = fsea_detail::check_n_frames(n_frames)) return rc;
    if (n_bytes && !bytes) return fail(FSEA_EINVAL, "NULL buffer");
    return FSEA_OK;
}

int check_output(const fsea_trace *t, int n_frames) {
    if ((size_t)n_frames > TR_MAX_OUT / frame_pixels(t)) return fail(FSEA_EINVAL, "%d frames are too many", n_frames);
    return FSEA_OK;
}

// the caller holds t->mu and is on t's device
int frames_launch(fsea_trace *t, const uint8_t *d_bytes, size_t n_bytes, int flip, size_t frame_bytes, int n_frames,
                  uint8_t *d_images, hipStream_t s) {
    if (n_frames == 0) return FSEA_OK;
    const TraceGeo &g = t->g;
    const size_t segments = (frame_bytes + 1) / 2 - 1;
    const int cb = segments <= 255 ? 1 : 4;
    const size_t plane = (size_t)g.side * g.side * cb;
    const size_t chunk = std::min<size_t>({(size_t)n_frames, (size_t)TR_MAX_CHUNK, std::max<size_t>(1, TR_COUNT_BYTES / plane)});
    // every use of the canvas and the planes, on whatever stream, follows the previous one
    if (int rc = t->counts.acquire(chunk * plane, s)) return rc;
    uint8_t *d_counts = static_cast<uint8_t *>(t->counts.buf.ptr);
    const size_t pixels = frame_pixels(t);
    const unsigned gx_hits = (unsigned)((segments + TR_WG - 1) / TR_WG);
    const unsigned gx_compose = (unsigned)(((pixels + 15) / 16 + TR_WG - 1) / TR_WG);
    const bool aligned = ((g.width | g.ox) & 15) == 0;
    const uint32_t fm = flip ? 0x80u : 0u;
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += chunk) {
        const int nf = (int)std::min(chunk, (size_t)n_frames - f0);
        FSEA_HIP(hipMemsetAsync(d_counts, 0, (size_t)nf * plane, s));
        const size_t first = f0 * frame_bytes;
        if (segments && first < n_bytes) {
            const dim3 grid(gx_hits, (unsigned)nf);
            const long long left = (long long)(n_bytes - first), fb = (long long)frame_bytes;
            uint32_t *counts = reinterpret_cast<uint32_t *>(d_counts);
            if (cb == 1) hipLaunchKernelGGL(fsea_trace_hits_b8, grid, dim3(TR_WG), 0, s, d_bytes + first, left, fb, fm, g, counts);
            else hipLaunchKernelGGL(fsea_trace_hits_b32, grid, dim3(TR_WG), 0, s, d_bytes + first, left, fb, fm, g, counts);
            FSEA_HIP(hipGetLastError());
        }
        uint8_t *images = d_images ? d_images + f0 * pixels : nullptr;
        const uint8_t *counts = d_counts;
        const dim3 grid(gx_compose);
        if (aligned && cb == 1) hipLaunchKernelGGL(fsea_trace_compose_b8, grid, dim3(TR_WG), 0, s, counts, nf, g, t->canvas.ptr, images);
        else if (aligned) hipLaunchKernelGGL(fsea_trace_compose_b32, grid, dim3(TR_WG), 0, s, counts, nf, g, t->canvas.ptr, images);
        else if (cb == 1) hipLaunchKernelGGL(fsea_trace_compose_b8_any, grid, dim3(TR_WG), 0, s, counts, nf, g, t->canvas.ptr, images);
        else hipLaunchKernelGGL(fsea_trace_compose_b32_any, grid, dim3(TR_WG), 0, s, counts, nf, g, t->canvas.ptr, images);
        FSEA_HIP(hipGetLastError());
    }
    return t->counts.release(s);
}

}  // namespace

extern "C" {

int fsea_trace_create(fsea_trace **out, const fsea_trace_config *cfg, int device) {
    if (!out) return fail(FSEA_EINVAL, "trace out-pointer is NULL");
    *out = nullptr;
    if (!cfg) return fail(FSEA_EINVAL, "trace config is NULL");
    const int m = cfg->size_multiplier;
    int rc = fsea_detail::check_multiplier(m);
    if (rc) return rc;
    if (cfg->width > TR_MAX_SIDE || cfg->height > TR_MAX_SIDE || IQ_RES * m > cfg->width || IQ_RES * m > cfg->height) {
        return fail(FSEA_EINVAL, "a %d x %d canvas does not hold the %d x %d IQ square (or is larger than %d)", cfg->width,
                    cfg->height, IQ_RES * m, IQ_RES * m, TR_MAX_SIDE);
    }
    if (cfg->pixel_inc < 1 || cfg->pixel_inc > 254) return fail(FSEA_EINVAL, "pixel_inc must be in [1, 254], got %d", cfg->pixel_inc);
    if (cfg->fade < 0 || cfg->fade > 255) return fail(FSEA_EINVAL, "fade must be in [0, 255], got %d", cfg->fade);
    return fsea_detail::create_object(out, device, "fsea_trace_create", [&](fsea_trace *t) {
        TraceGeo &g = t->g;
        g.width = cfg->width;
        g.height = cfg->height;
        g.m = m;
        g.side = IQ_RES * m;
        g.ox = (g.width - g.side) / 2;
        g.oy = (g.height - g.side) / 2;
        g.inc = cfg->pixel_inc;
        g.fade = cfg->fade;
        g.magic = (65536u + (uint32_t)g.inc - 1u) / (uint32_t)g.inc;
        t->canvas_bytes = (frame_pixels(t) + 15) & ~(size_t)15;
        hipError_t e = t->counts.create(t->staging.stream);
        if (e == hipSuccess) e = t->canvas.zeros(t->canvas_bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        return e;
    });
}

int fsea_trace_destroy(fsea_trace *t) { return fsea_detail::destroy_object(t); }

int fsea_trace_reset(fsea_trace *t) {
    return fsea_detail::reset_object(t, "trace is NULL", [&]() -> int {
        FSEA_HIP(t->canvas.zero(t->canvas_bytes));
        return FSEA_OK;
    });
}

int fsea_trace_frames_device(fsea_trace *t, const void *d_bytes, size_t n_bytes, int flip, size_t frame_bytes, int n_frames,
                             uint8_t *d_images, void *stream) {
    int rc = check_frames(t, d_bytes, n_bytes, frame_bytes, n_frames);
    if (!rc) rc = fsea_detail::check_aligned16("d_images", d_images);
    if (!rc) rc = check_output(t, n_frames);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    std::lock_guard<std::mutex> lock(t->mu);
    FSEA_ON_DEVICE(t->device);
    return frames_launch(t, static_cast<const uint8_t *>(d_bytes), n_bytes, flip, frame_bytes, n_frames, d_images,
                         static_cast<hipStream_t>(stream));
}

int fsea_trace_frames_host(fsea_trace *t, const void *bytes, size_t n_bytes, int flip, size_t frame_bytes, int n_frames,
                           uint8_t *images) {
    int rc = check_frames(t, bytes, n_bytes, frame_bytes, n_frames);
    if (!rc) rc = check_output(t, n_frames);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    // bytes behind the call's last point are never read
    const size_t used = std::min(n_bytes, (size_t)n_frames * frame_bytes + 1);
    std::lock_guard<std::mutex> lock(t->mu);
    FSEA_ON_DEVICE(t->device);
    return t->staging.run(
        used, images ? (size_t)n_frames * frame_pixels(t) : 0, images, [&](void *h_in) { std::memcpy(h_in, bytes, used); },
        [&](void *d_in, void *d_out, hipStream_t s) {
            return frames_launch(t, static_cast<const uint8_t *>(d_in), used, flip, frame_bytes, n_frames,
                                 images ? static_cast<uint8_t *>(d_out) : nullptr, s);
        });
}

int fsea_trace_canvas_host(fsea_trace *t, uint8_t *image) {
    if (!t) return fail(FSEA_EINVAL, "trace is NULL");
    if (!image) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(t->mu);
    FSEA_ON_DEVICE(t->device);
    const size_t pixels = frame_pixels(t);
    return t->staging.run(
        0, pixels, image, [](void *) {},
        [&](void *, void *d_out, hipStream_t s) {
            int rc = t->counts.acquire(s);
            if (rc) return rc;
            FSEA_HIP(hipMemcpyAsync(d_out, t->canvas.ptr, pixels, hipMemcpyDeviceToDevice, s));
            return t->counts.release(s);
        });
}

}  // extern "C"
