// fsea_plan_host.hip -- the host-buffer side of a plan (include/fsea.h): the fsea_exec_*_host entry points, small batches
// through mapped staging and large ones pipelined over three streams with the caller's pages pinned in place, and the
// device-resident history ring.  Everything here runs under the plan's host-path mutex and launches through
// fsea_detail::launch (fsea_plan.hip).
#include "../../include/fsea.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "fsea_registry.h"
#include "fsea_internal.h"

using namespace fsea_detail;

// ---- device-resident history ring (nrf_fft's history behind NRF_FFT_HISTORY=device) ----
struct fsea_history {
    fsea_plan *plan = nullptr;
    int device = 0;           // the plan's device (fsea_history_destroy must not need the plan any more)
    int rows = 0;
    int head = 0;             // ring row holding the newest spectrum
    int cur = 0;              // which of the two storages is live (nrf_fft_shift works out of place)
    DeviceArray<float> d_ring[2];
    PinnedArray<float> h_stage;   // rows * n floats: target of the D2H in fsea_history_get_f64
};

namespace {

// nrf_fft_shift on a device-resident history (src/nrf.c:569-596): every row moved by `shift` bins,
// vacated bins zero; out of place (src and dst are the two halves of the ring's ping-pong storage).
__global__ void fsea_history_shift_kernel(const float *src, float *dst, int n, size_t total, int shift) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % (size_t)n);
        const int from = x + shift;
        dst[i] = (from >= 0 && from < n) ? src[i - (size_t)x + (size_t)from] : 0.0f;
    }
}

__global__ void fsea_f64_to_f32_kernel(const double *in, float *out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        out[i] = (float)in[i];
    }
}

constexpr size_t FSEA_ZERO_COPY_MAX = 256 * 1024;  // in + out bytes up to which the staging is mapped host memory

// Pins the caller's buffer in place for the duration of one call, if the runtime lets us: copies from / to pinned pages
// are truly asynchronous (the two directions overlap: 2.56 instead of 3.57 ms for 64 MiB in + 128 MiB out on this box,
// profiles/r03_host_path.txt), pageable ones are staged by the runtime and return when done.  Memory that is pinned
// already (hipHostMalloc, fsea_host_alloc, registered by the caller) is left alone.
// Two host threads may hand the same buffer to two plans at once (one capture, two transform sizes): the registration is
// shared and counted, so that the first call to finish does not unpin pages the other one's copies are still using.
struct PinRegistry {
    struct Entry {
        void *ptr;
        size_t bytes;
        int users;
    };
    std::mutex mu;
    std::vector<Entry> live;
};
PinRegistry &pin_registry() {
    static PinRegistry r;
    return r;
}

struct PinnedInPlace {
    std::vector<void *> held;  // registrations this call keeps alive: its own, or those of calls in flight that it overlaps
    PinnedInPlace(const void *p, size_t bytes) {
        PinRegistry &r = pin_registry();
        std::lock_guard<std::mutex> lock(r.mu);
        const char *lo = static_cast<const char *>(p), *hi = lo + bytes;
        for (auto &e : r.live) {
            const char *elo = static_cast<const char *>(e.ptr), *ehi = elo + e.bytes;
            if (lo < ehi && elo < hi) {  // pinned (in part) by a call in flight on another thread: its pages must stay
                ++e.users;               // pinned until this call's copies are done as well
                held.push_back(e.ptr);
            }
        }
        if (!held.empty()) return;  // fully covered: asynchronous copies; partly: the runtime stages what is pageable
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type != hipMemoryTypeUnregistered) return;  // pinned or device
        (void)hipGetLastError();
        if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterDefault) == hipSuccess) {
            held.push_back(const_cast<void *>(p));
            r.live.push_back(PinRegistry::Entry{const_cast<void *>(p), bytes, 1});
        } else {
            (void)hipGetLastError();  // read-only mapping, foreign registration, ...: pageable copies still work
        }
    }
    ~PinnedInPlace() {
        if (held.empty()) return;
        PinRegistry &r = pin_registry();
        std::lock_guard<std::mutex> lock(r.mu);
        for (void *ptr : held) {
            for (size_t i = 0; i < r.live.size(); ++i) {
                if (r.live[i].ptr != ptr) continue;
                if (--r.live[i].users == 0) {
                    (void)hipHostUnregister(ptr);
                    r.live.erase(r.live.begin() + (long)i);
                }
                break;
            }
        }
    }
    PinnedInPlace(const PinnedInPlace &) = delete;
    PinnedInPlace &operator=(const PinnedInPlace &) = delete;
};

// Host-buffer execution, pipelined: the batch is cut into chunks of whole frames; chunk c's bytes travel on the copy-in
// stream while chunk c-1 is transformed on the plan's stream and chunk c-2's rows travel back on the copy-out stream
// (events order the three).  The streaming shape of the reference's tools (c/fft-batch.c:54-102: one transfer in, one
// row out) at the granularity a PCIe link wants.  bytes_per_sample: 2 (u8 IQ) or 16 (f64 IQ, narrowed on the device).
int exec_host_pipelined(fsea_plan *p, int in_kind, const void *in, size_t bytes_per_sample, size_t n_frames, int flip,
                        void *out, double rot_delta, double rot_phase0) {
    const size_t n = (size_t)p->n, hop = (size_t)p->hop;
    const size_t row_bytes = fsea_plan_row_bytes(p);
    const size_t n_samples = (n_frames - 1) * hop + n;
    const size_t in_bytes = n_samples * bytes_per_sample, out_bytes = n_frames * row_bytes;
    const bool f64 = bytes_per_sample == 16;
    int rc = (f64 ? p->host.d_aux : p->host.d_in).grow(in_bytes);
    if (rc) return rc;
    if (f64) {
        rc = p->host.d_in.grow(n_samples * 2 * sizeof(float));
        if (rc) return rc;
    }
    rc = p->host.d_out.grow(out_bytes);
    if (rc) return rc;
    // chunks of about 24 MiB (in + out): long enough for the link's full rate, short enough that the first copy-in and
    // the last copy-out (the two pieces nothing overlaps) are a small part of the call
    size_t chunks = (in_bytes + out_bytes) / ((size_t)24 << 20);
    if (chunks < 1) chunks = 1;
    if (chunks > FSEA_HOST_CHUNKS_MAX) chunks = FSEA_HOST_CHUNKS_MAX;
    size_t per = (n_frames + chunks - 1) / chunks;
    const size_t fpw = (size_t)p->entry->fpw;
    per = (per + fpw - 1) / fpw * fpw;  // whole units, so that a chunk boundary never splits a workgroup's frames
    chunks = (n_frames + per - 1) / per;
    PinnedInPlace pin_in(in, in_bytes), pin_out(out, out_bytes);
    auto run = [&]() -> int {
        const char *src = static_cast<const char *>(in);
        char *d_src = static_cast<char *>(f64 ? p->host.d_aux.ptr : p->host.d_in.ptr);
        size_t copied = 0;  // input bytes already on their way
        for (size_t c = 0; c < chunks; ++c) {
            const size_t f0 = c * per, f1 = (f0 + per < n_frames) ? f0 + per : n_frames;
            const size_t need = ((f1 - 1) * hop + n) * bytes_per_sample;  // everything chunk c reads (with its overlap into the next)
            if (need > copied) {
                FSEA_HIP(hipMemcpyAsync(d_src + copied, src + copied, need - copied, hipMemcpyHostToDevice, p->host.s_h2d));
                copied = need;
            }
            FSEA_HIP(hipEventRecord(p->host.ev_in[c], p->host.s_h2d));
            FSEA_HIP(hipStreamWaitEvent(p->stream, p->host.ev_in[c], 0));
            const char *d_frames = static_cast<const char *>(p->host.d_in.ptr) + f0 * hop * (f64 ? 2 * sizeof(float) : 2);
            if (f64) {
                const size_t v0 = f0 * hop * 2, v1 = ((f1 - 1) * hop + n) * 2;  // doubles of this chunk
                unsigned blocks = (unsigned)((v1 - v0 + 255) / 256);
                if (blocks > 2048) blocks = 2048;
                hipLaunchKernelGGL(fsea_f64_to_f32_kernel, dim3(blocks), dim3(256), 0, p->stream,
                                   static_cast<const double *>(p->host.d_aux.ptr) + v0, static_cast<float *>(p->host.d_in.ptr) + v0, v1 - v0);
            }
            const int lrc = launch(p, in_kind, d_frames, f1 - f0, flip, p->mode, static_cast<char *>(p->host.d_out.ptr) + f0 * row_bytes,
                                   p->stream, rot_delta, rot_phase0 + rot_delta * (double)(f0 * hop));
            if (lrc) return lrc;
            FSEA_HIP(hipEventRecord(p->host.ev_done[c], p->stream));
            FSEA_HIP(hipStreamWaitEvent(p->host.s_d2h, p->host.ev_done[c], 0));
            FSEA_HIP(hipMemcpyAsync(static_cast<char *>(out) + f0 * row_bytes, static_cast<char *>(p->host.d_out.ptr) + f0 * row_bytes,
                                    (f1 - f0) * row_bytes, hipMemcpyDeviceToHost, p->host.s_d2h));
        }
        FSEA_HIP(hipStreamSynchronize(p->host.s_d2h));
        return FSEA_OK;
    };
    rc = run();
    if (rc) {  // nothing of this call may still be using the caller's pages when they are unpinned
        (void)hipStreamSynchronize(p->host.s_h2d);
        (void)hipStreamSynchronize(p->stream);
        (void)hipStreamSynchronize(p->host.s_d2h);
    }
    return rc;
}

// `count` values into the mapped staging: f64 IQ narrowed to the f32 the transform reads, u8 IQ as it is
void fill_staging(void *h_in, const void *src, size_t count, bool f64) {
    if (!f64) {
        std::memcpy(h_in, src, count);
        return;
    }
    float *dst = static_cast<float *>(h_in);
    for (size_t i = 0; i < count; ++i) dst[i] = (float)static_cast<const double *>(src)[i];
}

// Common body of the host entry points: u8 IQ (bytes_per_sample 2), or f64 IQ (16) that reaches the transform as f32.
int exec_host(fsea_plan *p, int in_kind, const void *iq, size_t bytes_per_sample, size_t n_frames, int flip, void *out,
              double rot_delta, double rot_phase0) {
    if (!p) return fail(FSEA_EINVAL, "plan is NULL");
    if (n_frames == 0) return FSEA_OK;
    if (!iq || !out) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(p->host.mu);
    FSEA_ON_DEVICE(p->device);
    const bool f64 = bytes_per_sample == 16;
    const size_t n_values = 2 * ((n_frames - 1) * (size_t)p->hop + (size_t)p->n);
    const size_t in_bytes = n_values * (f64 ? sizeof(float) : 1);  // what the transform reads
    const size_t out_bytes = n_frames * fsea_plan_row_bytes(p);
    if (in_bytes + out_bytes <= FSEA_ZERO_COPY_MAX) {
        // small batch (nrf_fft_process on a samples or a shifter buffer): f64 is narrowed on the host, straight into the
        // mapped staging; one launch, one synchronisation
        return p->host.zero_copy(
            p->stream, in_bytes, out_bytes, out, [&](void *h_in) { fill_staging(h_in, iq, n_values, f64); },
            [&](const void *d_in, void *d_out) {
                return launch(p, in_kind, d_in, n_frames, flip, p->mode, d_out, p->stream, rot_delta, rot_phase0);
            });
    }
    return exec_host_pipelined(p, in_kind, iq, bytes_per_sample, n_frames, flip, out, rot_delta, rot_phase0);
}

// one frame from host memory, output row written straight into device memory
int push_frame(fsea_history *h, int in_kind, const void *host_in, size_t in_bytes, int flip) {
    fsea_plan *p = h->plan;
    std::lock_guard<std::mutex> lock(p->host.mu);
    FSEA_ON_DEVICE(p->device);
    const int new_head = (h->head + h->rows - 1) % h->rows;  // the ring head moves back by one
    float *row = h->d_ring[h->cur].ptr + (size_t)new_head * (size_t)p->n;
    const bool f64 = in_kind == fsea::IN_F32;
    auto fill = [&](void *h_in) { fill_staging(h_in, host_in, f64 ? in_bytes / sizeof(float) : in_bytes, f64); };
    // once it returns the staging is free again and the row is in place
    const int rc = p->host.zero_copy(p->stream, in_bytes, 0, nullptr, fill, [&](const void *d_in, void *) {
        return launch(p, in_kind, d_in, 1, flip, FSEA_MODE_MAG_F32, row, p->stream);
    });
    if (rc) return rc;
    h->head = new_head;
    return FSEA_OK;
}

}  // namespace

extern "C" {

int fsea_exec_u8_host(fsea_plan *p, const uint8_t *iq, size_t n_frames, int flip, void *out) {
    return exec_host(p, fsea::IN_U8, iq, 2, n_frames, flip, out, 0.0, 0.0);
}

int fsea_exec_u8_shifted_host(fsea_plan *p, const uint8_t *iq, size_t n_frames, int flip, double cycles_per_sample,
                              double phase0_cycles, void *out) {
    if (!std::isfinite(cycles_per_sample) || !std::isfinite(phase0_cycles)) {
        return fail(FSEA_EINVAL, "frequency shift must be finite");
    }
    return exec_host(p, fsea::IN_U8_ROT, iq, 2, n_frames, flip, out, cycles_per_sample, phase0_cycles);
}

int fsea_exec_f64_host(fsea_plan *p, const double *iq, size_t n_frames, void *out) {
    return exec_host(p, fsea::IN_F32, iq, 16, n_frames, 0, out, 0.0, 0.0);
}

int fsea_history_create(fsea_plan *p, int rows, fsea_history **out) {
    if (!out) return fail(FSEA_EINVAL, "history out-pointer is NULL");
    *out = nullptr;
    if (!p || rows <= 0) return fail(FSEA_EINVAL, "history needs a plan and a positive row count");
    if (p->mode != FSEA_MODE_MAG_F32) return fail(FSEA_EINVAL, "a history holds MAG_F32 rows");
    FSEA_ON_DEVICE(p->device);
    fsea_history *h = new (std::nothrow) fsea_history();
    if (!h) return fail(FSEA_ENOMEM, "out of host memory");
    h->plan = p;
    h->device = p->device;
    h->rows = rows;
    const size_t count = (size_t)rows * (size_t)p->n;
    hipError_t he = h->d_ring[0].zeros(count);
    if (he == hipSuccess) he = h->d_ring[1].alloc(count);
    if (he == hipSuccess) he = h->h_stage.alloc(count);
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) {
        int rc = fail(FSEA_EHIP, "history setup failed: %s", hipGetErrorString(he));
        delete h;
        return rc;
    }
    *out = h;
    return FSEA_OK;
}

int fsea_history_destroy(fsea_history *h) {
    if (!h) return FSEA_OK;
    DeviceGuard device_guard_(h->device);
    delete h;
    return FSEA_OK;
}

int fsea_history_push_u8_host(fsea_history *h, const uint8_t *iq, int flip) {
    if (!h || !iq) return fail(FSEA_EINVAL, "NULL argument");
    return push_frame(h, fsea::IN_U8, iq, 2 * (size_t)h->plan->n, flip);
}

int fsea_history_push_f64_host(fsea_history *h, const double *iq) {
    if (!h || !iq) return fail(FSEA_EINVAL, "NULL argument");
    return push_frame(h, fsea::IN_F32, iq, 2 * sizeof(float) * (size_t)h->plan->n, 0);
}

int fsea_history_shift(fsea_history *h, int shift) {
    if (!h) return fail(FSEA_EINVAL, "history is NULL");
    if (shift == 0) return FSEA_OK;
    fsea_plan *p = h->plan;
    std::lock_guard<std::mutex> lock(p->host.mu);
    FSEA_ON_DEVICE(p->device);
    const size_t total = (size_t)h->rows * (size_t)p->n;
    if (shift >= p->n || shift <= -p->n) {  // shifted out of range: start over (src/nrf.c:574-576)
        FSEA_HIP(hipMemsetAsync(h->d_ring[h->cur].ptr, 0, total * sizeof(float), p->stream));
    } else {
        unsigned blocks = (unsigned)((total + 255) / 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(fsea_history_shift_kernel, dim3(blocks), dim3(256), 0, p->stream, h->d_ring[h->cur].ptr,
                           h->d_ring[h->cur ^ 1].ptr, p->n, total, shift);
        FSEA_HIP(hipGetLastError());
        h->cur ^= 1;
    }
    FSEA_HIP(hipStreamSynchronize(p->stream));
    return FSEA_OK;
}

int fsea_history_get_f64(fsea_history *h, double *out) {
    if (!h || !out) return fail(FSEA_EINVAL, "NULL argument");
    fsea_plan *p = h->plan;
    std::lock_guard<std::mutex> lock(p->host.mu);
    FSEA_ON_DEVICE(p->device);
    const size_t n = (size_t)p->n;
    const size_t first = (size_t)(h->rows - h->head);  // rows from the head to the end of storage
    const float *ring = h->d_ring[h->cur].ptr;
    // one device-to-host transfer of rows * n f32, already in newest-first order, then one widening
    FSEA_HIP(hipMemcpyAsync(h->h_stage.ptr, ring + (size_t)h->head * n, first * n * sizeof(float), hipMemcpyDeviceToHost,
                            p->stream));
    if (h->head > 0) {
        FSEA_HIP(hipMemcpyAsync(h->h_stage.ptr + first * n, ring, (size_t)h->head * n * sizeof(float), hipMemcpyDeviceToHost,
                                p->stream));
    }
    FSEA_HIP(hipStreamSynchronize(p->stream));
    const size_t total = (size_t)h->rows * n;
    const float *src = h->h_stage.ptr;
    for (size_t i = 0; i < total; ++i) out[i] = (double)src[i];
    return FSEA_OK;
}

}  // extern "C"
