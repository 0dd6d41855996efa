// fsea_interp.hip -- blends of two resident sample blocks for an array of weights (include/fsea.h: fsea_interp_*): the
// batched form of the reference's nrf_interpolator_get_buffer (src/nrf.c:470-490) and of the frame loop of its movie tool
// (c/gradual-noise.c:96-112).
//
// Both kernels are store streams: a launch reads the two blocks (they stay in L2) and writes one frame per weight.  A
// workgroup reads its part of the blocks once, keeps it in registers (sample form) or LDS (image form) and writes that
// part of a run of frames; blockIdx.x, the part, runs fastest across the grid, so the workgroups in flight at one time
// write neighbouring parts of the same few frames.  Every store is a full 16-byte store to a 16-byte aligned address,
// except the bytes of a 16-byte group that a frame (sample form) or a tile of rows (image form) covers only in part.
//
// Sample form: lane g of the grid owns the 16 output bytes [16 g - s, 16 g - s + 16) of a frame, s the bytes by which the
// frame starts past a 16-byte boundary.  When the frame size is no multiple of 16 bytes, s differs between frames and
// repeats with period P = 16 / gcd(frame bytes, 16); a workgroup then writes frames p, p + P, p + 2 P, ... so that one
// s, and with it one set of elements per lane, serves its whole run.
//
// Image form ("The interpolator and the gradual-noise movie"): a workgroup owns a tile of image rows.
// Pixel (px, py) is the colour of sample (col[px], row[py]) (fsea_interp_image_tables), so the rows of a tile show few
// distinct sample rows ("slots").  Per frame the workgroup blends each slot's iq_size colours once into LDS; a lane then
// gathers 16 colours through the column table and stores them to every image row of that slot.  An image width that is no
// multiple of 16 takes the tile as one run of bytes instead and looks every byte up by itself.
#include "fsea_internal.h"

#include <algorithm>
#include <cstring>
#include <vector>

using fsea_detail::coord_f64;
using fsea_detail::DeviceGuard;
using fsea_detail::fail;

namespace {

constexpr int IT_WG = 256;
constexpr int IT_RUN = 8;            // frames per workgroup, sample form
constexpr int IM_RUN = 8;            // frames per workgroup, image form
constexpr int IM_MAX_ROWS = 16;      // image rows per tile at most
constexpr int IM_MAX_SIDE = 16384;   // image width and height at most
constexpr int IM_MAX_IQ = 4096;      // iq_size at most (the tables are u16)
constexpr size_t IM_MAX_LDS = 64 << 10;
constexpr size_t MAX_ELEMS = (size_t)1 << 31;
constexpr size_t MAX_OUT = (size_t)1 << 40;

template <int T> struct ElemBytes;
template <> struct ElemBytes<FSEA_IQ_U8> { static constexpr int v = 1; };
template <> struct ElemBytes<FSEA_IQ_F64> { static constexpr int v = 8; };

// element e of a block as the reference's nut_buffer_get_f64
template <int T>
__device__ __forceinline__ double load_elem(const void *__restrict__ p, long long e) {
    if (T == FSEA_IQ_U8) return (double)(static_cast<const uint8_t *>(p))[e] / 256.0;
    return (static_cast<const double *>(p))[e];
}

// grid (groups of 16 bytes / IT_WG, period x runs)
template <int T>
__device__ __forceinline__ void frames_body(const void *__restrict__ A, const void *__restrict__ B, long long n,
                                            const double *__restrict__ w, int n_frames, int period,
                                            uint8_t *__restrict__ out) {
#pragma clang fp contract(off)
    constexpr int ES = ElemBytes<T>::v;
    constexpr int EPG = 16 / ES;  // elements per 16-byte group
    const int phase = (int)(blockIdx.y % (unsigned)period);
    const long long first = (long long)(blockIdx.y / (unsigned)period) * IT_RUN;
    const long long nb = n * ES;
    const int s = (int)(((long long)phase * nb) & 15);  // a multiple of ES: `out` is 16-byte aligned
    const long long g = (long long)blockIdx.x * IT_WG + threadIdx.x;
    const long long e0 = (16 * g - s) / ES;  // first element of the group, negative in the frame's first group when s > 0
    if (e0 >= n) return;
    const bool full = e0 >= 0 && e0 + EPG <= n;

    double a[EPG], b[EPG];
    if (full && s == 0 && T == FSEA_IQ_U8) {
        const uint4 qa = (static_cast<const uint4 *>(A))[g], qb = (static_cast<const uint4 *>(B))[g];
        const uint32_t wa[4] = {qa.x, qa.y, qa.z, qa.w}, wb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
        for (int k = 0; k < EPG; ++k) {
            a[k] = (double)((wa[k >> 2] >> (8 * (k & 3))) & 0xffu) / 256.0;
            b[k] = (double)((wb[k >> 2] >> (8 * (k & 3))) & 0xffu) / 256.0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < EPG; ++k) {
            const bool ok = e0 + k >= 0 && e0 + k < n;
            a[k] = ok ? load_elem<T>(A, e0 + k) : 0.0;
            b[k] = ok ? load_elem<T>(B, e0 + k) : 0.0;
        }
    }

    for (int j = 0; j < IT_RUN; ++j) {
        const long long f = phase + (long long)period * (first + j);
        if (f >= n_frames) break;
        const double t = w[f];
        const double u = 1.0 - t;
        double v[EPG];
#pragma unroll
        for (int k = 0; k < EPG; ++k) v[k] = a[k] * u + b[k] * t;  // two products and a sum, each rounded
        uint8_t *dst = out + f * nb + (16 * g - s);  // 16-byte aligned: f * nb = s (mod 16)
        if (T == FSEA_IQ_U8) {
            uint32_t c[EPG];
#pragma unroll
            for (int k = 0; k < EPG; ++k) c[k] = coord_f64(v[k]);
            if (full) {
                uint32_t q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = c[4 * k] | c[4 * k + 1] << 8 | c[4 * k + 2] << 16 | c[4 * k + 3] << 24;
                *reinterpret_cast<uint4 *>(dst) = uint4{q[0], q[1], q[2], q[3]};
            } else {
#pragma unroll
                for (int k = 0; k < EPG; ++k) {
                    if (e0 + k >= 0 && e0 + k < n) dst[k] = (uint8_t)c[k];
                }
            }
        } else {
            if (full) {
                *reinterpret_cast<double2 *>(dst) = double2{v[0], v[EPG - 1]};
            } else {
#pragma unroll
                for (int k = 0; k < EPG; ++k) {
                    if (e0 + k >= 0 && e0 + k < n) reinterpret_cast<double *>(dst)[k] = v[k];
                }
            }
        }
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(IT_WG) void fsea_interp_frames_u8(const void *__restrict__ A,
                                                                          const void *__restrict__ B, long long n,
                                                                          const double *__restrict__ w, int n_frames,
                                                                          int period, uint8_t *__restrict__ out) {
    frames_body<FSEA_IQ_U8>(A, B, n, w, n_frames, period, out);
}
extern "C" __global__ __launch_bounds__(IT_WG) void fsea_interp_frames_f64(const void *__restrict__ A,
                                                                           const void *__restrict__ B, long long n,
                                                                           const double *__restrict__ w, int n_frames,
                                                                           int period, uint8_t *__restrict__ out) {
    frames_body<FSEA_IQ_F64>(A, B, n, w, n_frames, period, out);
}

// grid (tiles of `tile_rows` image rows, runs of IM_RUN frames); tab: the column table (width entries, padded to a multiple
// of 16) followed by the row table (height entries).  Dynamic LDS: the column table, then three arrays of
// max_slots x iq_size bytes (padded to 16): the slots' I bytes of A and of B, and their colours of the current frame.
extern "C" __global__ __launch_bounds__(IT_WG) void fsea_interp_image_u8(
    const uint8_t *__restrict__ A, const uint8_t *__restrict__ B, uint32_t flip, const double *__restrict__ w, int n_frames,
    int width, int height, int iq_size, int tile_rows, int max_slots, const uint16_t *__restrict__ tab,
    uint8_t *__restrict__ out) {
#pragma clang fp contract(off)
    extern __shared__ uint4 smem[];
    __shared__ int s_y[IM_MAX_ROWS], s_r0[IM_MAX_ROWS + 1], s_slot[IM_MAX_ROWS], s_slots;
    const int tid = threadIdx.x;
    const int w16 = (width + 15) & ~15, q16 = (iq_size + 15) & ~15;
    uint16_t *colx = reinterpret_cast<uint16_t *>(smem);
    uint8_t *sa = reinterpret_cast<uint8_t *>(colx + w16);
    uint8_t *sb = sa + (size_t)max_slots * q16;
    uint8_t *sc = sb + (size_t)max_slots * q16;
    const int py0 = (int)blockIdx.x * tile_rows;
    const int rows = min(tile_rows, height - py0);
    const long long f0 = (long long)blockIdx.y * IM_RUN;

    // the tile's slots: the row table does not decrease, so equal sample rows are neighbours
    if (tid == 0) {
        const uint16_t *rowtab = tab + w16;
        int D = 0;
        for (int r = 0; r < rows; ++r) {
            const int y = rowtab[py0 + r];
            if (r == 0 || y != s_y[D - 1]) {
                s_y[D] = y;
                s_r0[D] = r;
                ++D;
            }
            s_slot[r] = D - 1;
        }
        s_r0[D] = rows;
        s_slots = D;
    }
    for (int i = tid; i < w16; i += IT_WG) colx[i] = tab[i];
    __syncthreads();
    const int D = s_slots;
    for (int i = tid; i < D * iq_size; i += IT_WG) {
        const int d = i / iq_size, x = i - d * iq_size;
        const long long e = 2 * ((long long)s_y[d] * iq_size + x);  // the I byte of sample (x, y)
        sa[d * q16 + x] = (uint8_t)(A[e] ^ flip);
        sb[d * q16 + x] = (uint8_t)(B[e] ^ flip);
    }

    const size_t frame_bytes = (size_t)width * height;
    for (int j = 0; j < IM_RUN; ++j) {
        const long long f = f0 + j;
        if (f >= n_frames) break;
        const double t = w[f];
        const double u = 1.0 - t;
        __syncthreads();  // sa and sb are written; the previous frame's gathers are done with sc
        for (int i = tid; i < D * iq_size; i += IT_WG) {
            const int d = i / iq_size, x = i - d * iq_size;
            const double pwr = (double)sa[d * q16 + x] * u + (double)sb[d * q16 + x] * t;
            // the tool's clamp lets a NaN through, and x86-64's (int) of it has a zero low byte
            sc[d * q16 + x] = (uint8_t)(pwr != pwr ? 0 : (int)(pwr < 0.0 ? 0.0 : pwr > 255.0 ? 255.0 : pwr));
        }
        __syncthreads();
        if ((width & 15) == 0) {
            const int G = width >> 4;
            uint8_t *tile = out + (size_t)f * frame_bytes + (size_t)py0 * width;
            for (int i = tid; i < D * G; i += IT_WG) {
                const int d = i / G, g = i - d * G;
                const uint8_t *c = sc + d * q16;
                const uint4 i0 = reinterpret_cast<const uint4 *>(colx)[2 * g], i1 = reinterpret_cast<const uint4 *>(colx)[2 * g + 1];
                const uint32_t ix[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
                uint32_t q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    q[k] = (uint32_t)c[ix[2 * k] & 0xffffu] | (uint32_t)c[ix[2 * k] >> 16] << 8 |
                           (uint32_t)c[ix[2 * k + 1] & 0xffffu] << 16 | (uint32_t)c[ix[2 * k + 1] >> 16] << 24;
                }
                const uint4 v = uint4{q[0], q[1], q[2], q[3]};
                for (int r = s_r0[d]; r < s_r0[d + 1]; ++r) *reinterpret_cast<uint4 *>(tile + (size_t)r * width + 16 * g) = v;
            }
        } else {
            // the tile's rows as one run of bytes, in 16-byte groups of the output's own alignment
            const size_t begin = (size_t)f * frame_bytes + (size_t)py0 * width;
            const int s = (int)(begin & 15);
            const int nbytes = rows * width;
            uint8_t *base = out + (begin - s);
            for (int g = tid; 16 * g < s + nbytes; g += IT_WG) {
                uint32_t c[16];
                bool all = true;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int q = 16 * g - s + k;
                    const bool ok = q >= 0 && q < nbytes;
                    all = all && ok;
                    const int r = ok ? q / width : 0;
                    c[k] = ok ? sc[s_slot[r] * q16 + colx[q - r * width]] : 0u;
                }
                if (all) {
                    uint32_t q[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) q[k] = c[4 * k] | c[4 * k + 1] << 8 | c[4 * k + 2] << 16 | c[4 * k + 3] << 24;
                    *reinterpret_cast<uint4 *>(base + 16 * (size_t)g) = uint4{q[0], q[1], q[2], q[3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int q = 16 * g - s + k;
                        if (q >= 0 && q < nbytes) base[16 * (size_t)g + k] = (uint8_t)c[k];
                    }
                }
            }
        }
    }
}

struct fsea_interp {
    int device = 0;
    int type = FSEA_IQ_U8;
    size_t n = 0;                      // elements per block
    std::mutex mu;
    fsea_detail::DeviceArray<uint8_t> d_a, d_b;  // the blocks; a push copies into d_a's memory and swaps the two
    // the image form's tables on the device, for the geometry of the last call
    fsea_detail::SharedScratch tab;
    int tab_w = 0, tab_h = 0, tab_iq = 0, tile_rows = 0, max_slots = 0;
    fsea_detail::HostStaging staging;  // the host-buffer forms
};

namespace {

size_t elem_bytes(int type) { return type == FSEA_IQ_U8 ? 1 : 8; }

// The reference's scatter (put_block, put_pixel) in one dimension: which of the `iq_size` samples wrote pixel p of `side`
// last, -1 for none.  `scale` is the tool's BLOCK_SCALE; the double sum and its truncation to int are the tool's.
void last_writer(int side, int iq_size, double scale, int32_t *tab) {
    for (int p = 0; p < side; ++p) tab[p] = -1;
    for (int x = 0; x < iq_size; ++x) {
        for (int dx = 0; dx < scale; dx++) {
            const int p = (int)(x * scale + dx);
            if (p >= side) continue;
            tab[p] = x;
        }
    }
}

int check_geometry(int width, int height, int iq_size) {
    if (width < 1 || width > IM_MAX_SIDE || height < 1 || height > IM_MAX_SIDE) {
        return fail(FSEA_EINVAL, "image size %d x %d is outside [1, %d]", width, height, IM_MAX_SIDE);
    }
    if (iq_size < 1 || iq_size > IM_MAX_IQ) return fail(FSEA_EINVAL, "iq_size must be in [1, %d], got %d", IM_MAX_IQ, iq_size);
    return FSEA_OK;
}

double block_scale(int width, int height, int iq_size) {
    const double ws = width / (double)iq_size, hs = height / (double)iq_size;
    return ws > hs ? ws : hs;
}

size_t image_lds_bytes(int width, int iq_size, int max_slots) {
    return 2 * (size_t)((width + 15) & ~15) + 3 * (size_t)max_slots * (size_t)((iq_size + 15) & ~15);
}

int check_frames(const fsea_interp *p, int n_frames) {
    if (!p) return fail(FSEA_EINVAL, "interp is NULL");
    return fsea_detail::check_n_frames(n_frames);
}

int check_image(const fsea_interp *p, int n_frames, const fsea_interp_geometry *g) {
    int rc = check_frames(p, n_frames);
    if (rc) return rc;
    if (!g) return fail(FSEA_EINVAL, "geometry is NULL");
    rc = check_geometry(g->width, g->height, g->iq_size);
    if (rc) return rc;
    if (p->type != FSEA_IQ_U8) return fail(FSEA_EINVAL, "the image form needs FSEA_IQ_U8 blocks");
    if (p->n < 2 * (size_t)g->iq_size * g->iq_size) {
        return fail(FSEA_EINVAL, "blocks of %zu bytes hold no %d x %d IQ samples", p->n, g->iq_size, g->iq_size);
    }
    if ((size_t)n_frames > MAX_OUT / ((size_t)g->width * g->height)) return fail(FSEA_EINVAL, "%d frames are too many", n_frames);
    return FSEA_OK;
}

// the caller holds p->mu and is on p's device
int frames_launch(fsea_interp *p, const double *d_w, int n_frames, void *d_out, hipStream_t s) {
    if (n_frames == 0 || p->n == 0) return FSEA_OK;
    const long long n = (long long)p->n;
    const size_t nb = p->n * elem_bytes(p->type);
    int period = 1;
    while ((nb * period) & 15) period *= 2;
    const unsigned gx = (unsigned)((nb / 16 + 2 + IT_WG - 1) / IT_WG);  // a frame touches at most nb / 16 + 2 groups
    const int chunk = (65535 / period) * IT_RUN * period;               // frames of one launch: grid.y <= 65535
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        // f0 is a multiple of `period`: the chunk's frames start at the alignments of frames 0, 1, ...
        const int nf = std::min(chunk, n_frames - f0);
        const unsigned runs = (unsigned)(((nf + period - 1) / period + IT_RUN - 1) / IT_RUN);
        const dim3 grid(gx, (unsigned)period * runs);
        uint8_t *out = static_cast<uint8_t *>(d_out) + (size_t)f0 * nb;
        if (p->type == FSEA_IQ_U8) {
            hipLaunchKernelGGL(fsea_interp_frames_u8, grid, dim3(IT_WG), 0, s, p->d_a.ptr, p->d_b.ptr, n, d_w + f0, nf, period, out);
        } else {
            hipLaunchKernelGGL(fsea_interp_frames_f64, grid, dim3(IT_WG), 0, s, p->d_a.ptr, p->d_b.ptr, n, d_w + f0, nf, period, out);
        }
        FSEA_HIP(hipGetLastError());
    }
    return FSEA_OK;
}

// the tables of geometry g on the device (kept from the last call with the same geometry)
int image_tables(fsea_interp *p, const fsea_interp_geometry *g) {
    if (p->tab.buf.ptr && p->tab_w == g->width && p->tab_h == g->height && p->tab_iq == g->iq_size) return FSEA_OK;
    const int w16 = (g->width + 15) & ~15;
    std::vector<int32_t> col((size_t)g->width), row((size_t)g->height);
    const double scale = block_scale(g->width, g->height, g->iq_size);
    last_writer(g->width, g->iq_size, scale, col.data());
    last_writer(g->height, g->iq_size, scale, row.data());
    std::vector<uint16_t> tab((size_t)w16 + g->height, 0);
    for (int i = 0; i < g->width; ++i) {
        if (col[i] < 0) return fail(FSEA_EINVAL, "image column %d shows no sample", i);
        tab[i] = (uint16_t)col[i];
    }
    for (int i = 0; i < g->height; ++i) {
        if (row[i] < 0) return fail(FSEA_EINVAL, "image row %d shows no sample", i);
        tab[w16 + i] = (uint16_t)row[i];
    }
    // about two sample rows to a tile; the LDS holds the most distinct sample rows any tile shows
    const int tile_rows = std::max(1, std::min(IM_MAX_ROWS, (int)(2.0 * scale)));
    int max_slots = 1;
    for (int py0 = 0; py0 < g->height; py0 += tile_rows) {
        int slots = 1;
        for (int r = 1; r < tile_rows && py0 + r < g->height; ++r) slots += row[py0 + r] != row[py0 + r - 1];
        max_slots = std::max(max_slots, slots);
    }
    if (image_lds_bytes(g->width, g->iq_size, max_slots) > IM_MAX_LDS) {
        return fail(FSEA_EINVAL, "%d x %d images of %d x %d samples need more LDS than a workgroup has", g->width, g->height,
                    g->iq_size, g->iq_size);
    }
    int rc = p->tab.reserve(tab.size() * 2);  // no launch on any stream still reads the old tables
    if (rc) return rc;
    p->tab_w = 0;
    FSEA_HIP(hipMemcpy(p->tab.buf.ptr, tab.data(), tab.size() * 2, hipMemcpyHostToDevice));
    p->tab_w = g->width;
    p->tab_h = g->height;
    p->tab_iq = g->iq_size;
    p->tile_rows = tile_rows;
    p->max_slots = max_slots;
    return FSEA_OK;
}

int image_launch(fsea_interp *p, const double *d_w, int n_frames, const fsea_interp_geometry *g, void *d_images, hipStream_t s) {
    if (n_frames == 0) return FSEA_OK;
    int rc = image_tables(p, g);
    if (rc) return rc;
    const size_t lds = image_lds_bytes(g->width, g->iq_size, p->max_slots);
    const size_t frame_bytes = (size_t)g->width * g->height;
    const unsigned gx = (unsigned)((g->height + p->tile_rows - 1) / p->tile_rows);
    const int chunk = 65534 * IM_RUN;  // a multiple of 16 frames: every launch's images start 16-byte aligned
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = std::min(chunk, n_frames - f0);
        const dim3 grid(gx, (unsigned)((nf + IM_RUN - 1) / IM_RUN));
        hipLaunchKernelGGL(fsea_interp_image_u8, grid, dim3(IT_WG), lds, s, static_cast<const uint8_t *>(p->d_a.ptr),
                           static_cast<const uint8_t *>(p->d_b.ptr), g->flip ? 0x80u : 0u, d_w + f0, nf, g->width, g->height,
                           g->iq_size, p->tile_rows, p->max_slots, static_cast<const uint16_t *>(p->tab.buf.ptr),
                           static_cast<uint8_t *>(d_images) + (size_t)f0 * frame_bytes);
        FSEA_HIP(hipGetLastError());
    }
    return p->tab.release(s);
}

// B's old memory becomes A, the new block lands in A's old memory and becomes B
int push_launch(fsea_interp *p, const void *d_block, hipStream_t s) {
    const size_t nb = p->n * elem_bytes(p->type);
    if (nb) FSEA_HIP(hipMemcpyAsync(p->d_a.ptr, d_block, nb, hipMemcpyDeviceToDevice, s));
    std::swap(p->d_a.ptr, p->d_b.ptr);
    return FSEA_OK;
}

}  // namespace

extern "C" {

int fsea_interp_image_tables(int width, int height, int iq_size, int32_t *col, int32_t *row) {
    int rc = check_geometry(width, height, iq_size);
    if (rc) return rc;
    if (!col || !row) return fail(FSEA_EINVAL, "NULL table");
    const double scale = block_scale(width, height, iq_size);
    last_writer(width, iq_size, scale, col);
    last_writer(height, iq_size, scale, row);
    return FSEA_OK;
}

int fsea_interp_create(fsea_interp **out, int type, size_t n_elements, int device) {
    if (!out) return fail(FSEA_EINVAL, "interp out-pointer is NULL");
    *out = nullptr;
    if (type != FSEA_IQ_U8 && type != FSEA_IQ_F64) return fail(FSEA_EINVAL, "element type must be FSEA_IQ_U8 or FSEA_IQ_F64, got %d", type);
    if (n_elements > MAX_ELEMS) return fail(FSEA_EINVAL, "%zu elements are too many", n_elements);
    return fsea_detail::create_object(out, device, "fsea_interp_create", [&](fsea_interp *p) {
        p->type = type;
        p->n = n_elements;
        const size_t nb = std::max<size_t>(16, n_elements * elem_bytes(type));
        hipError_t e = p->tab.create(p->staging.stream);
        if (e == hipSuccess) e = p->d_a.zeros(nb);
        if (e == hipSuccess) e = p->d_b.zeros(nb);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        return e;
    });
}

int fsea_interp_destroy(fsea_interp *p) { return fsea_detail::destroy_object(p); }

// Not through fsea_detail::reset_object: without elements there is nothing to zero and no second wait.
int fsea_interp_reset(fsea_interp *p) {
    if (!p) return fail(FSEA_EINVAL, "interp is NULL");
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    FSEA_HIP(hipDeviceSynchronize());
    const size_t nb = p->n * elem_bytes(p->type);
    if (nb) {
        FSEA_HIP(p->d_a.zero(nb));
        FSEA_HIP(p->d_b.zero(nb));
        FSEA_HIP(hipDeviceSynchronize());
    }
    return FSEA_OK;
}

size_t fsea_interp_n_elements(const fsea_interp *p) { return p ? p->n : 0; }

int fsea_interp_push_device(fsea_interp *p, const void *d_block, void *stream) {
    if (!p) return fail(FSEA_EINVAL, "interp is NULL");
    if (p->n && !d_block) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return push_launch(p, d_block, static_cast<hipStream_t>(stream));
}

int fsea_interp_push_host(fsea_interp *p, const void *block) {
    if (!p) return fail(FSEA_EINVAL, "interp is NULL");
    if (p->n && !block) return fail(FSEA_EINVAL, "NULL buffer");
    const size_t nb = p->n * elem_bytes(p->type);
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return p->staging.run(
        nb, 0, nullptr, [&](void *h_in) { std::memcpy(h_in, block, nb); },
        [&](void *d_in, void *, hipStream_t s) { return push_launch(p, d_in, s); });
}

int fsea_interp_frames_device(fsea_interp *p, const double *d_weights, int n_frames, void *d_out, void *stream) {
    int rc = check_frames(p, n_frames);
    if (rc) return rc;
    if (n_frames == 0 || p->n == 0) return FSEA_OK;
    if (!d_weights || !d_out) return fail(FSEA_EINVAL, "NULL buffer");
    rc = fsea_detail::check_aligned16("d_out", d_out);
    if (rc) return rc;
    if ((uintptr_t)d_weights & 7) return fail(FSEA_EINVAL, "d_weights must be 8-byte aligned");
    if ((size_t)n_frames > MAX_OUT / (p->n * elem_bytes(p->type))) return fail(FSEA_EINVAL, "%d frames are too many", n_frames);
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return frames_launch(p, d_weights, n_frames, d_out, static_cast<hipStream_t>(stream));
}

int fsea_interp_frames_host(fsea_interp *p, const double *weights, int n_frames, void *out) {
    int rc = check_frames(p, n_frames);
    if (rc) return rc;
    if (n_frames == 0 || p->n == 0) return FSEA_OK;
    if (!weights || !out) return fail(FSEA_EINVAL, "NULL buffer");
    if ((size_t)n_frames > MAX_OUT / (p->n * elem_bytes(p->type))) return fail(FSEA_EINVAL, "%d frames are too many", n_frames);
    const size_t w_bytes = (size_t)n_frames * sizeof(double);
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return p->staging.run(
        w_bytes, (size_t)n_frames * p->n * elem_bytes(p->type), out, [&](void *h_in) { std::memcpy(h_in, weights, w_bytes); },
        [&](void *d_in, void *d_out, hipStream_t s) { return frames_launch(p, static_cast<const double *>(d_in), n_frames, d_out, s); });
}

int fsea_interp_image_frames_device(fsea_interp *p, const double *d_weights, int n_frames, const fsea_interp_geometry *g,
                                    void *d_images, void *stream) {
    int rc = check_image(p, n_frames, g);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    if (!d_weights || !d_images) return fail(FSEA_EINVAL, "NULL buffer");
    rc = fsea_detail::check_aligned16("d_images", d_images);
    if (rc) return rc;
    if ((uintptr_t)d_weights & 7) return fail(FSEA_EINVAL, "d_weights must be 8-byte aligned");
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return image_launch(p, d_weights, n_frames, g, d_images, static_cast<hipStream_t>(stream));
}

int fsea_interp_image_frames_host(fsea_interp *p, const double *weights, int n_frames, const fsea_interp_geometry *g,
                                  uint8_t *images) {
    int rc = check_image(p, n_frames, g);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    if (!weights || !images) return fail(FSEA_EINVAL, "NULL buffer");
    const size_t w_bytes = (size_t)n_frames * sizeof(double);
    std::lock_guard<std::mutex> lock(p->mu);
    FSEA_ON_DEVICE(p->device);
    return p->staging.run(
        w_bytes, (size_t)n_frames * g->width * g->height, images, [&](void *h_in) { std::memcpy(h_in, weights, w_bytes); },
        [&](void *d_in, void *d_out, hipStream_t s) { return image_launch(p, static_cast<const double *>(d_in), n_frames, g, d_out, s); });
}

}  // extern "C"
