// fsea_api.hip -- what every translation unit of libfsea_hip.so stands on, and the part of the C ABI (include/fsea.h) that
// takes no plan: the error plumbing, the bodies of the device objects' scaffold (fsea_internal.h), the job tables' upload
// kernel (fsea_jobs.h), device count, the alloc / copy / stream wrappers and the two image compositors.  Plans are in
// fsea_plan.hip and fsea_plan_host.hip.
#include "../../include/fsea.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "fsea_internal.h"
#include "fsea_jobs.h"

using namespace fsea_detail;

namespace {

thread_local std::string g_last_error = "";

__global__ void fsea_composite_max_kernel(uint8_t *dst, const uint8_t *src, uint32_t dst_x, uint32_t dst_y,
                                          uint32_t width, uint32_t height, uint32_t dst_stride,
                                          uint32_t src_stride) {
    // one thread per 4 horizontally adjacent pixels; rows by blockIdx.y
    const uint32_t x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    for (uint32_t y = blockIdx.y; y < height; y += gridDim.y) {
        if (x4 >= width) return;
        uint8_t *d = dst + (size_t)(dst_y + y) * dst_stride + dst_x + x4;
        const uint8_t *s = src + (size_t)y * src_stride + x4;
        const bool vec = (x4 + 4 <= width) && ((reinterpret_cast<uintptr_t>(d) & 3) == 0) &&
                         ((reinterpret_cast<uintptr_t>(s) & 3) == 0);
        if (vec) {
            const uint32_t a = *reinterpret_cast<const uint32_t *>(d);
            const uint32_t b = *reinterpret_cast<const uint32_t *>(s);
            uint32_t r = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t ab = (a >> (8 * k)) & 0xff, bb = (b >> (8 * k)) & 0xff;
                r |= (ab > bb ? ab : bb) << (8 * k);
            }
            *reinterpret_cast<uint32_t *>(d) = r;
        } else {
            for (uint32_t k = 0; k < 4 && x4 + k < width; ++k) d[k] = d[k] > s[k] ? d[k] : s[k];
        }
    }
}

// Many tiles in one launch: tile k (tiles contiguous, [k][y][x]) is max-composited at
// x0 + k*step.  Only tiles with k % stride_k == phase are touched, so that overlapping
// neighbours (step < width) are handled by separate launches without a race.
__global__ void fsea_stitch_tiles_kernel(uint8_t *dst, const uint8_t *tiles, uint32_t n_tiles, uint32_t x0,
                                         uint32_t step, uint32_t width, uint32_t height, uint32_t dst_stride,
                                         uint32_t stride_k, uint32_t phase) {
    const uint32_t k = (blockIdx.z * stride_k) + phase;
    if (k >= n_tiles) return;
    const uint32_t x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x4 >= width) return;
    for (uint32_t y = blockIdx.y; y < height; y += gridDim.y) {
        uint8_t *d = dst + (size_t)y * dst_stride + x0 + (size_t)k * step + x4;
        const uint8_t *s = tiles + ((size_t)k * height + y) * width + x4;
        const bool vec = (x4 + 4 <= width) && ((reinterpret_cast<uintptr_t>(d) & 3) == 0) &&
                         ((reinterpret_cast<uintptr_t>(s) & 3) == 0);
        if (vec) {
            const uint32_t a = *reinterpret_cast<const uint32_t *>(d);
            const uint32_t b = *reinterpret_cast<const uint32_t *>(s);
            uint32_t r = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t ab = (a >> (8 * q)) & 0xff, bb = (b >> (8 * q)) & 0xff;
                r |= (ab > bb ? ab : bb) << (8 * q);
            }
            *reinterpret_cast<uint32_t *>(d) = r;
        } else {
            for (uint32_t q = 0; q < 4 && x4 + q < width; ++q) d[q] = d[q] > s[q] ? d[q] : s[q];
        }
    }
}

}  // namespace

// A job table from the mapped host memory a call built it in to the device, one word a lane (fsea_jobs.h: JobTable)
extern "C" __global__ __launch_bounds__(256) void fsea_jobs_upload(const uint32_t *__restrict__ host, uint32_t *__restrict__ table,
                                                                 uint32_t n_words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_words) table[i] = host[i];
}

namespace fsea_detail {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int check_device(int device) {
    int count = 0;
    hipError_t ce = hipGetDeviceCount(&count);
    if (ce != hipSuccess || count <= 0) {
        return fail(FSEA_ENODEVICE, "no HIP device available (%s); libfsea_hip has no CPU fallback", hipGetErrorString(ce));
    }
    if (device < 0 || device >= count) return fail(FSEA_EINVAL, "device %d out of range [0,%d)", device, count);
    return FSEA_OK;
}

int check_multiplier(int size_multiplier) {
    if (size_multiplier < 1 || size_multiplier > FSEA_IQ_MAX_MULTIPLIER) {
        return fail(FSEA_EINVAL, "size_multiplier must be in [1, %d], got %d", FSEA_IQ_MAX_MULTIPLIER, size_multiplier);
    }
    return FSEA_OK;
}

int check_n_frames(int n_frames) {
    if (n_frames < 0) return fail(FSEA_EINVAL, "n_frames must be >= 0, got %d", n_frames);
    return FSEA_OK;
}

int check_aligned16(const char *names, const void *a, const void *b, const void *c) {
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) return fail(FSEA_EINVAL, "%s must be 16-byte aligned", names);
    return FSEA_OK;
}

int init_code(const char *what, hipError_t e) {
    return e == hipSuccess ? (int)FSEA_OK : fail(FSEA_EHIP, "%s: %s", what, hipGetErrorString(e));
}

int HostStaging::reserve(size_t in_bytes, size_t out_bytes) {
    // a buffer is freed only once the stream is idle: in the normal path it already is, but a call that returned an error
    // may have left a copy queued
    if ((h_in.ptr && h_in.cap < in_bytes) || (h_out.ptr && h_out.cap < out_bytes) || (d_in.ptr && d_in.cap < in_bytes) ||
        (d_out.ptr && d_out.cap < out_bytes)) {
        FSEA_HIP(hipStreamSynchronize(stream));
    }
    int rc = h_in.grow(in_bytes);
    if (!rc) rc = h_out.grow(out_bytes);
    if (!rc) rc = d_in.grow(in_bytes);
    if (!rc) rc = d_out.grow(out_bytes);
    return rc;
}

hipError_t SharedScratch::create(hipStream_t first) {
    const hipError_t e = used.create();
    return e == hipSuccess ? hipEventRecord(used, first) : e;
}

int SharedScratch::reserve(size_t need) {
    FSEA_HIP(hipEventSynchronize(used));  // no launch on any stream still uses the old buffer
    return buf.grow(need);
}

int SharedScratch::acquire(hipStream_t s) {
    FSEA_HIP(hipStreamWaitEvent(s, used, 0));
    return FSEA_OK;
}

int SharedScratch::acquire(size_t need, hipStream_t s) {
    const int rc = buf.cap < need ? reserve(need) : FSEA_OK;
    return rc ? rc : acquire(s);
}

int SharedScratch::release(hipStream_t s) {
    FSEA_HIP(hipEventRecord(used, s));
    return FSEA_OK;
}

int jobs_upload(const void *h_table, void *d_table, uint32_t n_words, hipStream_t s) {
    void *d_host = nullptr;
    FSEA_HIP(hipHostGetDevicePointer(&d_host, const_cast<void *>(h_table), 0));
    hipLaunchKernelGGL(fsea_jobs_upload, dim3((n_words + 255u) / 256u), dim3(256), 0, s, static_cast<const uint32_t *>(d_host),
                       static_cast<uint32_t *>(d_table), n_words);
    FSEA_HIP(hipGetLastError());
    return FSEA_OK;
}

}  // namespace fsea_detail

extern "C" {

const char *fsea_last_error_string(void) { return g_last_error.c_str(); }

int fsea_device_count(int *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (count) *count = (e == hipSuccess) ? n : 0;
    if (e != hipSuccess || n <= 0) return fail(FSEA_ENODEVICE, "no HIP device: %s", hipGetErrorString(e));
    return FSEA_OK;
}

int fsea_composite_max_device(void *d_dst, const void *d_src, uint32_t dst_x, uint32_t dst_y, uint32_t width,
                              uint32_t height, uint32_t dst_stride, uint32_t dst_height, uint32_t src_stride, int device,
                              void *stream) {
    if (!d_dst || !d_src) return fail(FSEA_EINVAL, "NULL buffer");
    if (width == 0 || height == 0) return FSEA_OK;
    if ((uint64_t)dst_x + (uint64_t)width > (uint64_t)dst_stride || width > src_stride) {
        return fail(FSEA_EINVAL, "tile does not fit the row stride");
    }
    if ((uint64_t)dst_y + (uint64_t)height > (uint64_t)dst_height) {
        return fail(FSEA_EINVAL, "tile rows %u..%llu do not fit the %u destination rows", dst_y,
                    (unsigned long long)dst_y + height, dst_height);
    }
    FSEA_ON_DEVICE(device);
    const unsigned bx = 64;
    dim3 grid((width / 4 + bx) / bx, height < 4096 ? height : 4096);
    hipLaunchKernelGGL(fsea_composite_max_kernel, grid, dim3(bx), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint8_t *>(d_dst), static_cast<const uint8_t *>(d_src), dst_x, dst_y, width, height,
                       dst_stride, src_stride);
    FSEA_HIP(hipGetLastError());
    return FSEA_OK;
}

int fsea_stitch_tiles_device(void *d_image, const void *d_tiles, uint32_t n_tiles, uint32_t first_x,
                             uint32_t width_step, uint32_t width, uint32_t height, uint32_t image_stride, int device,
                             void *stream) {
    if (!d_image || !d_tiles) return fail(FSEA_EINVAL, "NULL buffer");
    if (n_tiles == 0 || width == 0 || height == 0) return FSEA_OK;
    if (width_step == 0) return fail(FSEA_EINVAL, "width_step must be positive");
    if ((size_t)first_x + (size_t)(n_tiles - 1) * width_step + width > image_stride) {
        return fail(FSEA_EINVAL, "tiles do not fit the image row stride");
    }
    FSEA_ON_DEVICE(device);
    // tiles k and k + m overlap when m * step < width: m phases keep every launch race-free
    const uint32_t phases = (width + width_step - 1) / width_step;
    const unsigned bx = 64;
    for (uint32_t ph = 0; ph < phases; ++ph) {
        const uint32_t cnt = (n_tiles > ph) ? (n_tiles - ph + phases - 1) / phases : 0;
        if (cnt == 0) continue;
        dim3 grid((width / 4 + bx) / bx, height < 1024 ? height : 1024, cnt);
        hipLaunchKernelGGL(fsea_stitch_tiles_kernel, grid, dim3(bx), 0, static_cast<hipStream_t>(stream),
                           static_cast<uint8_t *>(d_image), static_cast<const uint8_t *>(d_tiles), n_tiles, first_x,
                           width_step, width, height, image_stride, phases, ph);
    }
    FSEA_HIP(hipGetLastError());
    return FSEA_OK;
}

int fsea_device_alloc(int device, size_t bytes, void **d_ptr) {
    if (!d_ptr) return fail(FSEA_EINVAL, "NULL out-pointer");
    FSEA_ON_DEVICE(device);
    FSEA_HIP(hipMalloc(d_ptr, bytes ? bytes : 16));
    return FSEA_OK;
}

int fsea_device_free(int device, void *d_ptr) {
    if (!d_ptr) return FSEA_OK;
    FSEA_ON_DEVICE(device);
    FSEA_HIP(hipFree(d_ptr));
    return FSEA_OK;
}

int fsea_host_alloc(size_t bytes, void **ptr) {
    if (!ptr) return fail(FSEA_EINVAL, "NULL out-pointer");
    *ptr = nullptr;
    FSEA_HIP(hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocPortable));
    return FSEA_OK;
}

int fsea_host_free(void *ptr) {
    if (!ptr) return FSEA_OK;
    FSEA_HIP(hipHostFree(ptr));
    return FSEA_OK;
}

int fsea_copy_to_device(int device, void *d_dst, const void *src, size_t bytes) {
    FSEA_ON_DEVICE(device);
    FSEA_HIP(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return FSEA_OK;
}

int fsea_copy_to_host(int device, void *dst, const void *d_src, size_t bytes) {
    FSEA_ON_DEVICE(device);
    FSEA_HIP(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return FSEA_OK;
}

int fsea_stream_create(int device, void **stream) {
    if (!stream) return fail(FSEA_EINVAL, "stream out-pointer is NULL");
    *stream = nullptr;
    FSEA_ON_DEVICE(device);
    hipStream_t s = nullptr;
    FSEA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return FSEA_OK;
}

int fsea_stream_destroy(int device, void *stream) {
    if (!stream) return FSEA_OK;
    FSEA_ON_DEVICE(device);
    FSEA_HIP(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return FSEA_OK;
}

int fsea_copy_to_device_async(int device, void *d_dst, const void *src, size_t bytes, void *stream) {
    FSEA_ON_DEVICE(device);
    FSEA_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    return FSEA_OK;
}

int fsea_copy_to_host_async(int device, void *dst, const void *d_src, size_t bytes, void *stream) {
    FSEA_ON_DEVICE(device);
    FSEA_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    return FSEA_OK;
}

int fsea_stream_synchronize(fsea_plan *p, void *stream) {
    if (!p) return fail(FSEA_EINVAL, "plan is NULL");
    FSEA_ON_DEVICE(p->device);
    FSEA_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return FSEA_OK;
}

}  // extern "C"
