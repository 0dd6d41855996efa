// fsea_plan.hip -- the FFT plan of the C ABI (include/fsea.h) on device buffers.
//
// Host-side plan management around the kernels of fsea_fft_core.h: the kernel registry, twiddle tables, a plan's life
// cycle, persistent-grid sizing, the ticket-counter slots, launches, the taper window, the mean-magnitude reduction and
// the tuning library's entry points.  No CPU compute path exists here: if HIP cannot give us a device, plan creation
// fails.  The host-buffer entry points are in fsea_plan_host.hip.
#include "../../include/fsea.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "fsea_registry.h"
#include "fsea_tables.h"
#include "fsea_internal.h"

using namespace fsea_detail;

extern "C" int fsea_kernels_small(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_alt(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_1024(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_2048(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_4096(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_8192(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_16384(fsea::KernelEntry *out, int cap);
#ifdef FSEA_TUNE  // libfsea_hip_tune.so: the product kernels plus the tuning variants and ablations
#include "../../include/fsea_tune.h"
extern "C" int fsea_kernels_tune_8192a(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_8192b(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_abl(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_mid(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_px(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_big(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_w64(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_lay(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_pw(fsea::KernelEntry *out, int cap);
extern "C" int fsea_kernels_tune_win(fsea::KernelEntry *out, int cap);
#endif

// ---- what the parts of a plan own (fsea_internal.h) ----
hipError_t fsea_plan::Counters::create() { return d_ctr.zeros(FSEA_CTR_SLOTS * FSEA_CTR_WORDS); }

hipError_t fsea_plan::HostPath::create() {
    hipError_t he = s_h2d.create();
    if (he == hipSuccess) he = s_d2h.create();
    for (unsigned c = 0; c < FSEA_HOST_CHUNKS_MAX && he == hipSuccess; ++c) {
        he = ev_in[c].create();
        if (he == hipSuccess) he = ev_done[c].create();
    }
    return he;
}

#ifdef FSEA_TUNE
// A plain stream with the headline kernel's byte mix, 1 read : 2 written, and its cache policy (nt both ways): every thread
// moves 16 bytes in and 32 bytes out per iteration.  What the memory system gives a kernel that does nothing else.
typedef uint32_t tune_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void fsea_tune_stream_1to2_kernel(const tune_u32x4 *in, tune_u32x4 *out, size_t n16) {
    // four independent 16-byte loads in flight per thread, every wave instruction 1 KiB contiguous in both directions
    // (the two output halves are two contiguous streams, as the rows of two frames would be)
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        tune_u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __builtin_nontemporal_load(in + i + k * stride);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tune_u32x4 w = v[k];
            w.x ^= 0x80808080u;
            __builtin_nontemporal_store(v[k], out + i + k * stride);
            __builtin_nontemporal_store(w, out + n16 + i + k * stride);
        }
    }
    for (; i < n16; i += stride) {
        const tune_u32x4 v = __builtin_nontemporal_load(in + i);
        tune_u32x4 w = v;
        w.x ^= 0x80808080u;
        __builtin_nontemporal_store(v, out + i);
        __builtin_nontemporal_store(w, out + n16 + i);
    }
}
#endif

namespace {

const std::vector<fsea::KernelEntry> &registry() {
    static std::vector<fsea::KernelEntry> all = [] {
        std::vector<fsea::KernelEntry> v;
        fsea::KernelEntry tmp[32];
        int (*lists[])(fsea::KernelEntry *, int) = {fsea_kernels_small, fsea_kernels_alt, fsea_kernels_1024, fsea_kernels_2048,
                                                    fsea_kernels_4096,  fsea_kernels_8192, fsea_kernels_16384,
#ifdef FSEA_TUNE
                                                    fsea_kernels_tune_8192a, fsea_kernels_tune_8192b,
                                                    fsea_kernels_tune_abl, fsea_kernels_tune_px, fsea_kernels_tune_mid, fsea_kernels_tune_big,
                                                    fsea_kernels_tune_w64, fsea_kernels_tune_lay, fsea_kernels_tune_pw, fsea_kernels_tune_win,
#endif
        };
        for (auto fn : lists) {
            int n = fn(tmp, 32);
            for (int i = 0; i < n; ++i) v.push_back(tmp[i]);
        }
        return v;
    }();
    return all;
}

const fsea::KernelEntry *find_entry(int n, const char *variant) {
    for (const auto &e : registry()) {
        if (e.n == n && std::strcmp(e.variant, variant ? variant : "") == 0) return &e;
    }
    return nullptr;
}

// Which __global__ entry point of the plan's configuration serves (input kind, epilogue mode, byte convention); -1, with
// the error set, where the variant has none.
int select_kind(const fsea_plan *p, int in_kind, int mode, int flip) {
    const fsea::KernelEntry *e = p->entry;
    int kind = fsea::K_U8;
    if (in_kind == fsea::IN_F32) kind = fsea::K_F32;
    else if (in_kind == fsea::IN_U8_ROT) kind = fsea::K_U8_ROT;
    else if (flip && mode == FSEA_MODE_MAG_F32) kind = fsea::K_U8_MAG;
    else if (flip && mode == FSEA_MODE_DB5_U8_DCFIX) kind = fsea::K_U8_DB5;
    else if (flip && mode == FSEA_MODE_DB10_U8) kind = fsea::K_U8_DB10;
    if (p->window.form != 0) {
        // a plan with a taper launches the windowed twin; for the frequency-shifted and f32 inputs that is the
        // nrf_freq_shifter -> nrf_fft chain and the F64 branch of nrf_fft_process (src/nrf.c:607-612) with the taper
        static const int twin[] = {fsea::K_U8_MAG_WIN, fsea::K_U8_DB5_WIN, fsea::K_U8_DB10_WIN,
                                   fsea::K_U8_WIN,     fsea::K_U8_ROT_WIN, fsea::K_F32_WIN};
        kind = twin[kind];
    }
    // tuning variants carry the u8 MAG and run-time-mode kernels only: their pixel modes run the latter
    if (!e->fn[kind] && in_kind == fsea::IN_U8) kind = p->window.form != 0 ? fsea::K_U8_WIN : fsea::K_U8;
    if (!e->fn[kind]) {
        fail(FSEA_EINVAL, "kernel variant '%s' has no entry point for this input kind", e->variant);
        return -1;
    }
    return kind;
}

// The half-overlap twin of MAG kind `kind` when this launch runs it, else -1: 50 %-overlapped frames of the
// nrf_fft_process kind (raw int8, MAG rows) at the sizes with one frame per workgroup, not tiled, two frames or more.
int half_overlap_kind(const fsea_plan *p, int kind, size_t n_frames, bool tiled) {
    const int half = kind == fsea::K_U8_MAG ? fsea::K_U8_MAG_HALF : kind == fsea::K_U8_MAG_WIN ? fsea::K_U8_MAG_HALF_WIN : -1;
    if (half < 0 || !p->entry->fn[half] || tiled || n_frames < 2 || 2 * (size_t)p->hop != (size_t)p->n || p->no_half_overlap) {
        return -1;
    }
    return half;
}

// Every kind of every configuration takes one FftArgs by value (FSEA_KERNEL_FN_); the caller reads the launch's status
// with hipGetLastError.
void launch_kind(const fsea::KernelEntry *e, int kind, fsea::FftArgs &a, unsigned grid, hipStream_t s) {
    void *args[] = {&a};
    (void)hipLaunchKernel(e->fn[kind], dim3(grid), dim3(e->wg), args, 0, s);
}

__global__ void fsea_sum_f32_kernel(const float *x, size_t n, double *acc) {
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        s += (double)x[i];
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double part[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) part[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) tot += part[i];
        atomicAdd(acc, tot);
    }
}

// the kernel raw int8 input (flip) launches on a plan of a size with kernels of its own; whether that is the half-overlap
// kernel is decided as for a typical launch (two frames or more, not tiled)
std::string pow2_kernel_name(const fsea_plan *p) {
    const int k = select_kind(p, fsea::IN_U8, p->mode, 1);
    if (k < 0) return "";
    const int half = half_overlap_kind(p, k, 2, false);
    return p->entry->name[half >= 0 ? half : k];
}

unsigned grid_for(const fsea_plan *p, const fsea::KernelEntry *e, int occ, size_t n_frames) {
    const size_t units = (n_frames + e->fpw - 1) / e->fpw;
    size_t g = (size_t)p->num_cu * (size_t)(occ > 0 ? occ : 1);
    if (units < g) g = units;
    if (g >= 8) g &= ~(size_t)7;  // the kernel's XCD-aware frame mapping wants a multiple of 8
    if (g == 0) g = 1;
    return (unsigned)g;
}

// The ticket-counter slot for a launch on stream `s` that uses the counters (see fsea_plan::d_ctr).
//  * A stream keeps its slot: launches on one stream run in order and the last workgroup of a launch zeroes the slot.
//  * A slot is handed to another stream once the event recorded behind its last launch has completed (least recently
//    used first), so a plan may see any number of short-lived streams over its lifetime; with FSEA_CTR_SLOTS launches in
//    flight on as many streams, the call waits for the oldest of them instead of failing.
//  * A stream handle that matches a slot whose last launch is still running is either that stream (already ordered) or a
//    new stream that got a destroyed stream's handle: the launch is ordered behind the slot's event either way.
//  * hipStreamPerThread names a different stream in every thread: it never keeps a slot, every launch takes a free one.
//  * While `s` is being captured into a graph nothing but the kernel may be enqueued: no event; the slot then stays
//    with that stream handle for good (replay one instance of such a graph at a time, include/fsea.h).
// Returns null only if an event cannot be created or every slot belongs to a captured stream.
unsigned *counter_slot(fsea_plan *p, hipStream_t s, int *index, bool *record) {
    std::lock_guard<std::mutex> lock(p->ctr.slot_mu);
    bool capturing = false;
    if (s != nullptr) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) == hipSuccess) capturing = (st == hipStreamCaptureStatusActive);
        else (void)hipGetLastError();
    }
    const bool anonymous = (s == hipStreamPerThread);
    int pick = -1;
    if (!anonymous) {
        for (unsigned i = 0; i < FSEA_CTR_SLOTS; ++i) {
            if (p->ctr.slots[i].used && !p->ctr.slots[i].anonymous && p->ctr.slots[i].stream == s) pick = (int)i;
        }
        if (pick >= 0 && p->ctr.slots[pick].pending && !capturing) {
            if (hipStreamWaitEvent(s, p->ctr.slots[pick].ev, 0) != hipSuccess) (void)hipGetLastError();
        }
    }
    if (pick < 0) {
        for (unsigned i = 0; i < FSEA_CTR_SLOTS && pick < 0; ++i) {
            if (!p->ctr.slots[i].used) pick = (int)i;
        }
        int oldest = -1;
        for (unsigned i = 0; i < FSEA_CTR_SLOTS && pick < 0; ++i) {
            fsea_plan::Counters::Slot &c = p->ctr.slots[i];
            if (c.captured || c.launching) continue;  // launching: claimed by another host thread whose kernel is being enqueued
            if (!c.pending || hipEventQuery(c.ev) == hipSuccess) {
                if (pick < 0 || c.seq < p->ctr.slots[pick].seq) pick = (int)i;
            } else {
                (void)hipGetLastError();  // hipErrorNotReady is not an error
                if (oldest < 0 || c.seq < p->ctr.slots[oldest].seq) oldest = (int)i;
            }
        }
        if (pick < 0 && oldest >= 0) {  // FSEA_CTR_SLOTS launches in flight: wait for the oldest one
            if (hipEventSynchronize(p->ctr.slots[oldest].ev) != hipSuccess) return nullptr;
            pick = oldest;
        }
        if (pick < 0) return nullptr;
        p->ctr.slots[pick].used = true;
        p->ctr.slots[pick].pending = false;
        p->ctr.slots[pick].anonymous = anonymous;
        p->ctr.slots[pick].stream = s;
    }
    fsea_plan::Counters::Slot &c = p->ctr.slots[pick];
    // A slot a capture has used stays reserved for its stream until fsea_plan_reset: an instantiated hipGraph has the slot's
    // counter address baked into its kernel node, so recycling it to another stream (round 4 did, once the capturing stream
    // launched un-captured again) would let a replay share one counter with that stream's launches.  The
    // capturing stream itself keeps using it for ordinary launches, in stream order with a replay on that stream.
    if (capturing) c.captured = true;
    if (!capturing && !c.ev) {
        if (c.ev.create() != hipSuccess) return nullptr;
    }
    c.seq = ++p->ctr.slot_seq;
    c.launching = true;  // until launch_pow2 has enqueued the kernel and recorded the slot's event
    *index = pick;
    *record = !capturing;
    return p->ctr.d_ctr.ptr + (size_t)FSEA_CTR_WORDS * (size_t)pick;
}

int launch_pow2(fsea_plan *p, int in_kind, const void *d_in, size_t n_frames, int flip, int mode, void *d_out,
                hipStream_t s, double rot_delta, double rot_phase0, const TileLayout *tiles) {
    if (n_frames == 0) return FSEA_OK;
    const int kind = select_kind(p, in_kind, mode, flip);
    if (kind < 0) return FSEA_EINVAL;
    const fsea::KernelEntry *e = p->entry;
    fsea::FftArgs a;
    a.win = p->window.d_win.ptr;
    a.win_dc = p->window.d_win_dc.ptr;
    a.win_offset = p->window.form == 2 ? 1u : 0u;
    a.rot_delta = rot_delta;
    a.rot_phase0 = rot_phase0;
    if (in_kind == fsea::IN_U8_ROT) {
        fsea::TwPair rows[32];
        fsea::build_rotation_rows(p->n, e->radix[0], rot_delta, rows);
        for (int r = 0; r < 32; ++r) a.rot_row[r] = fsea::cf{rows[r].re, rows[r].im};
    }
    a.in = d_in;
    a.out = d_out;
    a.n_frames = n_frames;
    a.hop = (size_t)p->hop;
    a.xormask = flip ? 0u : 0x80808080u;
    a.mode = mode;
    a.trace = p->d_trace.ptr;
    for (int i = 0; i < 4; ++i) a.tw[i] = p->d_tw.ptr + p->tw_off[i];
    a.tw_small = p->d_tw.ptr;
    a.tw_def = p->d_tw.ptr + p->tw_def_off;
    // units per workgroup of this launch: few -> static interleave, many -> ticket pools (FftArgs::dynamic_units)
    {
        const unsigned grid = grid_for(p, e, p->occ[kind], n_frames);
        const size_t n_units = (n_frames + (size_t)e->fpw - 1) / (size_t)e->fpw;
        a.dynamic_units = p->units_policy == FSEA_UNITS_TICKETS  ? 1u
                          : p->units_policy == FSEA_UNITS_STATIC ? 0u
                                                                 : (n_units > (size_t)FSEA_STATIC_UNITS_PER_WG * grid ? 1u : 0u);
    }
    if (tiles) {
        a.tile_rows = tiles->rows;
        a.pitch_row = tiles->pitch_row;
        a.pitch_tile = tiles->pitch_tile;
        a.out_span = tiles->span;
    }
    // the half-overlap kernel: runs of consecutive frames per workgroup (every sample loaded once), static units
    const int half_kind = half_overlap_kind(p, kind, n_frames, tiles != nullptr);
    if (half_kind >= 0) {
        const size_t wgs = (size_t)p->num_cu * (size_t)(p->occ[half_kind] > 0 ? p->occ[half_kind] : 1);
        size_t run = (n_frames + wgs - 1) / wgs;  // frames per run: long enough to reuse most halves, short enough that every workgroup gets some
        if (run > (size_t)p->half_run_max) run = (size_t)p->half_run_max;
        if (run < 1) run = 1;
        a.run_len = (uint32_t)run;
        a.dynamic_units = 0;
        a.ctr = p->ctr.d_ctr.ptr;
        const size_t units = (n_frames + run - 1) / run;
        size_t g = wgs < units ? wgs : units;
        if (g >= 8) g &= ~(size_t)7;
        launch_kind(e, half_kind, a, (unsigned)g, s);
        FSEA_HIP(hipGetLastError());
        return FSEA_OK;
    }
    // only a launch that hands its frames out by the ticket pools needs a counter slot (single-wave sizes and short
    // launches never touch the counters)
    int slot = -1;
    bool record = false;
    a.ctr = p->ctr.d_ctr.ptr;
    if (e->counters == 2 || (e->counters == 1 && a.dynamic_units != 0)) {
        a.ctr = counter_slot(p, s, &slot, &record);
        if (!a.ctr) {
            return fail(FSEA_EHIP, "no ticket-counter slot for this launch: all %u slots of the plan are reserved by streams with captured "
                                   "launches (fsea_plan_release_stream once a stream's graphs are destroyed, or fsea_plan_reset), or an "
                                   "event could not be created", FSEA_CTR_SLOTS);
        }
    }
    launch_kind(e, kind, a, grid_for(p, e, p->occ[kind], n_frames), s);
    const hipError_t launched = hipGetLastError();
    if (slot >= 0) {
        std::lock_guard<std::mutex> lock(p->ctr.slot_mu);
        p->ctr.slots[slot].launching = false;
        if (record && launched == hipSuccess) {
            FSEA_HIP(hipEventRecord(p->ctr.slots[slot].ev, s));
            p->ctr.slots[slot].pending = true;
        }
    }
    if (launched != hipSuccess) return fail(FSEA_EHIP, "kernel launch failed: %s", hipGetErrorString(launched));
    return FSEA_OK;
}

int check_exec_args(const fsea_plan *plan, const void *in, const void *out, size_t align) {
    if (!plan) return fail(FSEA_EINVAL, "plan is NULL");
    if (!in || !out) return fail(FSEA_EINVAL, "NULL buffer");
    if (reinterpret_cast<uintptr_t>(in) % align) return fail(FSEA_EINVAL, "input pointer must be %zu-byte aligned", align);
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(FSEA_EINVAL, "output pointer must be 16-byte aligned");
    return FSEA_OK;
}

// Not through create_object (fsea_internal.h): a plan has no HostStaging, it needs the device's properties before it is
// allocated, and its setup failure has a text of its own.
int create_plan(fsea_plan **out, int fft_size, int hop, int mode, int device, const char *variant) {
    if (!out) return fail(FSEA_EINVAL, "plan out-pointer is NULL");
    *out = nullptr;
    if (mode < FSEA_MODE_MAG_F32 || mode > FSEA_MODE_DB_F32) return fail(FSEA_EINVAL, "unknown mode %d", mode);
    const fsea::KernelEntry *e = find_entry(fft_size, variant);
    int blu_m = 0, fs_n1 = 0, fs_n2 = 0;
    if (!e) {
        if (variant && variant[0]) {
            return fail(FSEA_EINVAL, "no kernel variant '%s' for fft_size %d", variant, fft_size);
        }
        // a size FFTW takes and no kernel has: a power of two above 16384 in two passes of the kernels (four-step), anything
        // else by Bluestein's algorithm on a power of two m >= 2n - 1
        if (fourstep_split(fft_size, &fs_n1, &fs_n2)) {
            e = find_entry(fs_n1, "");
        } else {
            blu_m = bluestein_m(fft_size);
            if (blu_m) e = find_entry(blu_m <= 16384 ? blu_m : 16384, "");
        }
        if (!e) {
            return fail(FSEA_EINVAL, "unsupported fft_size %d: the gfx950 kernels cover powers of two in [32, 16384] directly, larger "
                                     "powers of two up to %d in two passes, and every other size from 2 to %d through Bluestein's "
                                     "algorithm", fft_size, FSEA_MAX_FFT_SIZE, (FSEA_MAX_FFT_SIZE + 1) / 2);
        }
    }
    if (hop <= 0 || (!blu_m && !fs_n1 && (hop % 8) != 0)) {
        return fail(FSEA_EINVAL, "hop must be a positive multiple of 8 (any positive hop for the sizes without a kernel of their "
                                 "own); got %d", hop);
    }
    int rc = check_device(device);
    if (rc) return rc;
    FSEA_ON_DEVICE(device);
    hipDeviceProp_t prop;
    FSEA_HIP(hipGetDeviceProperties(&prop, device));

    fsea_plan *p = new (std::nothrow) fsea_plan();
    if (!p) return fail(FSEA_ENOMEM, "out of host memory");
    p->n = fft_size;
    p->hop = hop;
    p->mode = mode;
    p->device = device;
    p->entry = e;
    p->blu.m = blu_m;
    p->fs.n1 = fs_n1;
    p->fs.n2 = fs_n2;
    p->num_cu = prop.multiProcessorCount;
    p->no_half_overlap = std::getenv("FSEA_NO_HALF_OVERLAP") != nullptr;
    if (const char *hr = std::getenv("FSEA_HALF_RUN_MAX")) {
        const int v = std::atoi(hr);
        if (v >= 1 && v <= 4096) p->half_run_max = v;
    }
    p->kernel_name = pow2_kernel_name(p);
#ifdef FSEA_TUNE
    if (std::getenv("FSEA_TRACE")) {
        if (p->d_trace.alloc(4096 * 32) != hipSuccess) p->d_trace.ptr = nullptr;
    }
#endif

    std::vector<fsea::TwPair> tw;
    fsea::build_twiddles(e->np, e->radix, tw, p->tw_off);
    {
        std::vector<fsea::TwPair> def;
        fsea::build_deferred_table(e->radix[0], e->radix[1], def);
        if (tw.size() & 1) tw.push_back(fsea::TwPair{0.f, 0.f});
        p->tw_def_off = tw.size();
        tw.insert(tw.end(), def.begin(), def.end());
    }
    hipError_t he = p->d_tw.upload(tw.data(), tw.size());
    if (he == hipSuccess) he = p->stream.create();
    if (he == hipSuccess) he = p->host.d_acc.alloc(1);
    if (he == hipSuccess) he = p->ctr.create();
    // the counters' memset runs on the null stream; the caller's (possibly non-blocking) streams are not ordered
    // behind it, so it is complete before the plan is handed out
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he == hipSuccess) he = p->ev0.create(hipEventDefault);
    if (he == hipSuccess) he = p->ev1.create(hipEventDefault);
    if (he == hipSuccess) he = p->host.create();
    for (int k = 0; k < fsea::K_COUNT && he == hipSuccess; ++k) {
        if (e->fn[k]) he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&p->occ[k], e->fn[k], e->wg, 0);
    }
    if (he != hipSuccess) {
        rc = fail(FSEA_EHIP, "plan setup failed: %s", hipGetErrorString(he));
        delete p;
        return rc;
    }
    if (blu_m) {
        rc = create_plan(&p->blu.inner.ptr, blu_m, blu_m, FSEA_MODE_COMPLEX_F32, device, "");
        if (rc == FSEA_OK) rc = blu_setup(p);
        if (rc != FSEA_OK) {
            delete p;
            return rc;
        }
        p->kernel_name = std::string("bluestein(") +
                         (p->blu.inner->fs.n1 ? p->blu.inner->kernel_name : std::string(p->blu.inner->entry->name[fsea::K_F32])) + " x2)";
    }
    if (fs_n1) {
        rc = create_plan(&p->fs.inner1.ptr, fs_n1, fs_n1, FSEA_MODE_COMPLEX_F32, device, "");
        if (rc == FSEA_OK) rc = create_plan(&p->fs.inner2.ptr, fs_n2, fs_n2, FSEA_MODE_COMPLEX_F32, device, "");
        if (rc == FSEA_OK) rc = fs_setup(p);
        if (rc != FSEA_OK) {
            delete p;
            return rc;
        }
        p->kernel_name = std::string("fourstep(") + p->fs.inner1->entry->name[fsea::K_F32] + ", " + p->fs.inner2->entry->name[fsea::K_F32] + ")";
    }
    *out = p;
    return FSEA_OK;
}

// The configuration a plan of (fft_size, mode) takes where the modes of a size prefer different radix orders
// (fsea_configs.h: FSEA_CFG_256_ROWS, FSEA_CFG_512_PX, FSEA_CFG_1024_RT); "" = the size's first configuration.
const char *preferred_variant(int fft_size, int mode) {
    const bool f32_rows = mode == FSEA_MODE_MAG_F32 || mode == FSEA_MODE_MAG_NODC_F32 || mode == FSEA_MODE_DB_F32;
    const bool pixels = mode == FSEA_MODE_DB10_U8 || mode == FSEA_MODE_DB5_U8_DCFIX;
    if (fft_size == 256 && f32_rows) return "rows";
    if (fft_size == 512 && pixels) return "px";
    // 1024 points: the modes only the run-time-mode kernel serves (COMPLEX_F32, MAG_NODC_F32, DB_F32)
    if (fft_size == 1024 && (mode == FSEA_MODE_COMPLEX_F32 || mode == FSEA_MODE_MAG_NODC_F32 || mode == FSEA_MODE_DB_F32)) return "rt";
    return "";
}

#ifdef FSEA_TUNE
// `reps` calls of body(i), which queues work on `s`, between the events e0 and e1: their average time in ms
template <class Body>
int time_reps(hipEvent_t e0, hipEvent_t e1, hipStream_t s, int reps, float *avg_ms, Body &&body) {
    FSEA_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < reps; ++i) {
        const int rc = body(i);
        if (rc) return rc;
    }
    FSEA_HIP(hipEventRecord(e1, s));
    FSEA_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FSEA_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / (float)reps;
    return FSEA_OK;
}
#endif

}  // namespace

namespace fsea_detail {

size_t mode_elem_bytes(int mode) {
    switch (mode) {
    case FSEA_MODE_DB10_U8:
    case FSEA_MODE_DB5_U8_DCFIX:
        return 1;
    case FSEA_MODE_COMPLEX_F32:
        return 8;
    default:
        return 4;
    }
}

int launch(fsea_plan *p, int in_kind, const void *d_in, size_t n_frames, int flip, int mode, void *d_out,
           hipStream_t s, double rot_delta, double rot_phase0, const TileLayout *tiles) {
    if (p->blu.m || p->fs.n1) {
        if (in_kind == fsea::IN_U8_ROT || tiles) {
            return fail(FSEA_EINVAL, "fft_size %d runs through %s: the frequency-shifted and the tiled "
                                     "entry points exist for the power-of-two sizes from 32 to 16384 only", p->n,
                        p->blu.m ? "Bluestein's algorithm" : "the four-step decomposition");
        }
        if (s != nullptr) {  // five to ten launches through the plan's own work buffers, ordered by events: not capturable
            hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive) {
                return fail(FSEA_EINVAL, "fft_size %d runs through %s, whose launches cannot be captured into a graph (include/fsea.h); "
                                         "only the powers of two from 32 to 16384 can", p->n,
                            p->blu.m ? "Bluestein's algorithm" : "the four-step decomposition");
            }
            (void)hipGetLastError();
        }
        std::lock_guard<std::mutex> lock(p->work.mu);
        if (!p->work.ev) FSEA_HIP(p->work.ev.create());
        if (p->work.pending) FSEA_HIP(hipStreamWaitEvent(s, p->work.ev, 0));
        const int rc = p->blu.m ? blu_launch(p, in_kind, d_in, n_frames, flip, mode, d_out, s)
                                : fs_launch(p, in_kind, d_in, n_frames, flip, mode, d_out, s);
        FSEA_HIP(hipEventRecord(p->work.ev, s));
        p->work.pending = true;
        return rc;
    }
    return launch_pow2(p, in_kind, d_in, n_frames, flip, mode, d_out, s, rot_delta, rot_phase0, tiles);
}

}  // namespace fsea_detail

extern "C" {

int fsea_plan_create(fsea_plan **out, int fft_size, int hop, int mode, int device) {
    const char *variant = std::getenv("FSEA_ONE_CONFIG_PER_SIZE") ? "" : preferred_variant(fft_size, mode);  // (A/B measurements)
    if (variant[0] && !find_entry(fft_size, variant)) variant = "";
    return create_plan(out, fft_size, hop, mode, device, variant);
}

// Recovery: waits for the device and zeroes every ticket-counter slot (a launch that was aborted
// leaves its slot non-zero, which would make later launches on that stream skip or repeat frames).
int fsea_plan_reset(fsea_plan *p) {
    if (!p) return fail(FSEA_EINVAL, "plan is NULL");
    FSEA_ON_DEVICE(p->device);
    FSEA_HIP(hipDeviceSynchronize());
    FSEA_HIP(p->ctr.d_ctr.zero(FSEA_CTR_SLOTS * FSEA_CTR_WORDS));
    FSEA_HIP(hipDeviceSynchronize());
    {
        std::lock_guard<std::mutex> lock(p->ctr.slot_mu);
        for (auto &c : p->ctr.slots) c.used = c.pending = c.anonymous = c.captured = c.launching = false;
    }
    return FSEA_OK;
}

// Gives back the ticket-counter slot `stream` holds in this plan -- in particular one reserved by a captured launch -- once
// the graphs captured on that stream are destroyed (an application that captures on short-lived streams would
// otherwise run out of the 64 slots).  Waits for the slot's last un-captured launch; the slot's counters are left as every
// finished launch leaves them (zero).  FSEA_OK also when the stream holds no slot.
int fsea_plan_release_stream(fsea_plan *p, void *stream) {
    if (!p) return fail(FSEA_EINVAL, "plan is NULL");
    FSEA_ON_DEVICE(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (s != nullptr) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive) {
            return fail(FSEA_EINVAL, "fsea_plan_release_stream: the stream is being captured");
        }
        (void)hipGetLastError();
    }
    std::lock_guard<std::mutex> lock(p->ctr.slot_mu);
    for (auto &c : p->ctr.slots) {
        if (!c.used || c.anonymous || c.stream != s) continue;
        if (c.launching) return fail(FSEA_EINVAL, "fsea_plan_release_stream: another thread is launching on this stream");
        if (c.pending && c.ev) FSEA_HIP(hipEventSynchronize(c.ev));
        c.used = c.pending = c.captured = false;
    }
    return FSEA_OK;
}

int fsea_plan_destroy(fsea_plan *p) {
    if (!p) return FSEA_OK;
    DeviceGuard device_guard_(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;  // every part frees what it owns, inner plans included
    return FSEA_OK;
}

size_t fsea_plan_row_bytes(const fsea_plan *p) { return p ? (size_t)p->n * mode_elem_bytes(p->mode) : 0; }
int fsea_plan_fft_size(const fsea_plan *p) { return p ? p->n : 0; }
const char *fsea_plan_kernel_name(const fsea_plan *p) {
    if (!p) return "";
    return (p->window.form != 0 && !p->kernel_name_win.empty()) ? p->kernel_name_win.c_str() : p->kernel_name.c_str();
}

int fsea_plan_set_unit_distribution(fsea_plan *p, int policy) {
    if (!p) return fail(FSEA_EINVAL, "plan is NULL");
    if (policy != FSEA_UNITS_AUTO && policy != FSEA_UNITS_STATIC && policy != FSEA_UNITS_TICKETS) {
        return fail(FSEA_EINVAL, "unknown unit distribution %d", policy);
    }
    p->units_policy = policy;
    return FSEA_OK;
}

int fsea_window_fill(int kind, int n, float *w) {
    static const double coef[6][5] = {{1.0, 0, 0, 0, 0},
                                      {0.5, 0.5, 0, 0, 0},
                                      {0.54, 0.46, 0, 0, 0},
                                      {0.42, 0.5, 0.08, 0, 0},
                                      {0.35875, 0.48829, 0.14128, 0.01168, 0},
                                      {0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368}};
    if (kind < FSEA_WINDOW_RECT || kind > FSEA_WINDOW_FLATTOP) return fail(FSEA_EINVAL, "unknown window kind %d", kind);
    if (n < 1 || !w) return fail(FSEA_EINVAL, "fsea_window_fill: n >= 1 and a buffer of n floats");
    const double tau = 6.283185307179586476925286766559;
    for (int j = 0; j < n; ++j) {
        double v = 0.0, sign = 1.0;
        for (int k = 0; k < 5; ++k) {
            if (coef[kind][k] != 0.0) v += sign * coef[kind][k] * std::cos(tau * (double)k * (double)j / (double)n);
            sign = -sign;
        }
        w[j] = (float)v;
    }
    return FSEA_OK;
}

int fsea_plan_window_form(const fsea_plan *p) { return p ? p->window.form : 0; }

int fsea_plan_set_window(fsea_plan *p, const float *w) {
    if (!p) return fail(FSEA_EINVAL, "plan is NULL");
    if (p->blu.m || p->fs.n1) {
        return fail(FSEA_EINVAL, "fft_size %d has no kernel of its own (Bluestein / four-step path): the taper window is fused into "
                                 "the kernels of the powers of two from 32 to 16384", p->n);
    }
    const fsea::KernelEntry *e = p->entry;
    FSEA_ON_DEVICE(p->device);
    FSEA_HIP(hipDeviceSynchronize());  // no launch of this plan may still be reading the tables that are replaced
    if (!w) {
        p->window.form = 0;
        return FSEA_OK;
    }
    if (!e->fn[fsea::K_U8_WIN] || !e->fn[fsea::K_U8_MAG_WIN]) {
        return fail(FSEA_EINVAL, "kernel variant '%s' of size %d has no windowed kernels", e->variant, p->n);
    }
    const int n = p->n;
    for (int j = 0; j < n; ++j) {
        if (!std::isfinite(w[j])) return fail(FSEA_EINVAL, "window weight %d is not finite", j);
    }
    std::vector<float> perm;
    std::vector<fsea::TwPair> dc;
    const int form = fsea::build_window_tables(n, e->t, e->radix[0], e->radix[e->np - 1], w, perm, dc);
    if (!p->window.d_win.ptr) FSEA_HIP(p->window.d_win.alloc((size_t)n));
    if (!p->window.d_win_dc.ptr) FSEA_HIP(p->window.d_win_dc.alloc(dc.size()));
    FSEA_HIP(hipMemcpy(p->window.d_win.ptr, perm.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    FSEA_HIP(hipMemcpy(p->window.d_win_dc.ptr, dc.data(), dc.size() * sizeof(fsea::cf), hipMemcpyHostToDevice));
    p->window.form = form;
    // computed once: everything pow2_kernel_name reads (entry, mode, hop, no_half_overlap) is fixed at plan creation
    // (FSEA_NO_HALF_OVERLAP is read there, not per launch), so the windowed name cannot go stale
    if (p->kernel_name_win.empty()) p->kernel_name_win = pow2_kernel_name(p);
    return FSEA_OK;
}

int fsea_plan_grid(const fsea_plan *p, size_t n_frames, unsigned *grid, unsigned *block, size_t *lds_bytes) {
    if (!p) return fail(FSEA_EINVAL, "plan is NULL");
    // the kernel raw int8 input (flip) launches -- for a hop == N/2 plan the ordinary MAG kernel's geometry, not the
    // half-overlap kernel's, as this call has always reported
    const int k = select_kind(p, fsea::IN_U8, p->mode, 1);
    if (k < 0) return FSEA_EINVAL;
    if (grid) *grid = grid_for(p, p->entry, p->occ[k], n_frames);
    if (block) *block = (unsigned)p->entry->wg;
    // a plan with a taper launches the *_WIN kernels, whose static LDS carries the DC table on top
    if (lds_bytes) *lds_bytes = p->entry->lds_bytes[k];
    return FSEA_OK;
}

int fsea_exec_u8_device(fsea_plan *p, const void *d_iq, size_t n_frames, int flip, void *d_out, void *stream) {
    int rc = check_exec_args(p, d_iq, d_out, 16);
    if (rc) return rc;
    FSEA_ON_DEVICE(p->device);
    return launch(p, fsea::IN_U8, d_iq, n_frames, flip, p->mode, d_out,
                  static_cast<hipStream_t>(stream));
}

int fsea_exec_u8_tiled_device(fsea_plan *p, const void *d_iq, size_t n_frames, int flip, void *d_image,
                              size_t image_rows, size_t image_stride, size_t first_x, size_t tile_rows, size_t tile_step,
                              void *stream) {
    int rc = check_exec_args(p, d_iq, d_image, 16);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    const size_t n = (size_t)p->n, esz = fsea_plan_row_bytes(p) / n;
    const int fpw = p->entry->fpw;
    if (tile_rows == 0 || tile_rows > image_rows) return fail(FSEA_EINVAL, "tile_rows must be in [1, image_rows]");
    if (tile_rows % (size_t)fpw != 0) {
        return fail(FSEA_EINVAL, "tile_rows must be a multiple of %d at fft_size %d (frames per workgroup)", fpw, p->n);
    }
    if (n_frames % tile_rows != 0) return fail(FSEA_EINVAL, "n_frames must be whole tiles (a multiple of tile_rows)");
    if (tile_step < n) return fail(FSEA_EINVAL, "tile_step must be at least fft_size: tiles are written, not max-composited");
    if ((image_stride | first_x | tile_step) % 4 != 0) {
        return fail(FSEA_EINVAL, "image_stride, first_x and tile_step must be multiples of 4 elements");
    }
    const size_t n_tiles = n_frames / tile_rows;
    if (first_x + (n_tiles - 1) * tile_step + n > image_stride) return fail(FSEA_EINVAL, "tiles leave the image row");
    const size_t span = image_rows * image_stride - first_x;
    if (n_frames > 0xffffffffull || image_stride > 0xffffffffull || tile_step > 0xffffffffull ||
        ((size_t)(fpw - 1) * image_stride + n) * esz > 0xffffffffull) {
        return fail(FSEA_EINVAL, "image geometry exceeds the kernel's 32-bit row offsets");
    }
    TileLayout t;
    t.rows = (uint32_t)tile_rows;
    t.pitch_row = (uint32_t)image_stride;
    t.pitch_tile = (uint32_t)tile_step;
    t.span = span;
    FSEA_ON_DEVICE(p->device);
    return launch(p, fsea::IN_U8, d_iq, n_frames, flip, p->mode, static_cast<char *>(d_image) + first_x * esz,
                  static_cast<hipStream_t>(stream), 0.0, 0.0, &t);
}

int fsea_exec_u8_shifted_device(fsea_plan *p, const void *d_iq, size_t n_frames, int flip, double cycles_per_sample,
                                double phase0_cycles, void *d_out, void *stream) {
    int rc = check_exec_args(p, d_iq, d_out, 16);
    if (rc) return rc;
    if (!std::isfinite(cycles_per_sample) || !std::isfinite(phase0_cycles)) {
        return fail(FSEA_EINVAL, "frequency shift must be finite");
    }
    FSEA_ON_DEVICE(p->device);
    return launch(p, fsea::IN_U8_ROT, d_iq, n_frames, flip, p->mode, d_out, static_cast<hipStream_t>(stream),
                  cycles_per_sample, phase0_cycles);
}

int fsea_mean_magnitude_u8_device(fsea_plan *p, const void *d_iq, size_t n_frames, int flip, double *mean,
                                  void *stream) {
    if (!p || !mean) return fail(FSEA_EINVAL, "NULL argument");
    if (!d_iq) return fail(FSEA_EINVAL, "NULL buffer");
    if (n_frames == 0) {
        *mean = 0.0;
        return FSEA_OK;
    }
    std::lock_guard<std::mutex> lock(p->host.mu);
    FSEA_ON_DEVICE(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t count = n_frames * (size_t)p->n;
    int rc = p->host.d_aux.grow(count * sizeof(float));
    if (rc) return rc;
    rc = launch(p, fsea::IN_U8, d_iq, n_frames, flip, FSEA_MODE_MAG_NODC_F32, p->host.d_aux.ptr, s);
    if (rc) return rc;
    FSEA_HIP(hipMemsetAsync(p->host.d_acc.ptr, 0, sizeof(double), s));
    unsigned blocks = (unsigned)((count + 1023) / 1024);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(fsea_sum_f32_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const float *>(p->host.d_aux.ptr), count,
                       p->host.d_acc.ptr);
    double total = 0.0;
    FSEA_HIP(hipMemcpyAsync(&total, p->host.d_acc.ptr, sizeof(double), hipMemcpyDeviceToHost, s));
    FSEA_HIP(hipStreamSynchronize(s));
    *mean = total / (double)count;
    return FSEA_OK;
}

#ifdef FSEA_TUNE
// ---- tuning / measurement entry points (include/fsea_tune.h; libfsea_hip_tune.so only) ----
int fsea_tune_stream_1to2(void *const *d_in, void *const *d_out, int n_sets, size_t in_bytes, int device, void *stream,
                          int reps, float *avg_ms) {
    if (!d_in || !d_out || n_sets <= 0 || reps <= 0 || !avg_ms || (in_bytes % 16) != 0) return fail(FSEA_EINVAL, "bad arguments");
    FSEA_ON_DEVICE(device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipDeviceProp_t prop;
    FSEA_HIP(hipGetDeviceProperties(&prop, device));
    Event e0, e1;
    FSEA_HIP(e0.create(hipEventDefault));
    FSEA_HIP(e1.create(hipEventDefault));
    const char *wg_env = std::getenv("FSEA_TUNE_COPY_WG");  // workgroups per CU (default 32: two 16-byte pieces per thread; measured 0.58-0.67 of 8 TB/s at 2-16, 0.73 at 32)
    const unsigned grid = (unsigned)prop.multiProcessorCount * (unsigned)(wg_env ? std::atoi(wg_env) : 32);
    return time_reps(e0, e1, s, reps, avg_ms, [&](int i) {
        hipLaunchKernelGGL(fsea_tune_stream_1to2_kernel, dim3(grid), dim3(256), 0, s, static_cast<const tune_u32x4 *>(d_in[i % n_sets]),
                           static_cast<tune_u32x4 *>(d_out[i % n_sets]), in_bytes / 16);
        return (int)FSEA_OK;
    });
}

int fsea_plan_create_variant(fsea_plan **out, int fft_size, int hop, int mode, int device, const char *variant) {
    return create_plan(out, fft_size, hop, mode, device, variant ? variant : "");
}

// Diagnostics (FSEA_TRACE=1): copies the [grid][32] trace words of the last launch.
int fsea_plan_read_trace(fsea_plan *p, unsigned long long *out, unsigned n_workgroups) {
    if (!p || !p->d_trace.ptr || n_workgroups > 4096) return fail(FSEA_EINVAL, "tracing is not enabled for this plan");
    FSEA_ON_DEVICE(p->device);
    FSEA_HIP(hipMemcpy(out, p->d_trace.ptr, (size_t)n_workgroups * 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FSEA_OK;
}

int fsea_time_exec_u8_device(fsea_plan *p, const void *d_iq, size_t n_frames, int flip, void *d_out, void *stream,
                             int reps, float *avg_ms) {
    int rc = check_exec_args(p, d_iq, d_out, 16);
    if (rc) return rc;
    if (reps <= 0 || !avg_ms) return fail(FSEA_EINVAL, "reps must be > 0 and avg_ms non-NULL");
    FSEA_ON_DEVICE(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return time_reps(p->ev0, p->ev1, s, reps, avg_ms,
                     [&](int) { return launch(p, fsea::IN_U8, d_iq, n_frames, flip, p->mode, d_out, s); });
}

// The same over n_sets independent buffer sets used in rotation, so that no launch finds its
// bytes in the 256 MiB Infinity Cache (the streaming regime bench.py measures).
int fsea_time_exec_u8_rotating(fsea_plan *p, void *const *d_iq, void *const *d_out, int n_sets, size_t n_frames,
                               int flip, void *stream, int reps, float *avg_ms) {
    if (!p || !d_iq || !d_out || n_sets <= 0 || reps <= 0 || !avg_ms) return fail(FSEA_EINVAL, "bad arguments");
    FSEA_ON_DEVICE(p->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return time_reps(p->ev0, p->ev1, s, reps, avg_ms, [&](int i) {
        return launch(p, fsea::IN_U8, d_iq[i % n_sets], n_frames, flip, p->mode, d_out[i % n_sets], s);
    });
}
#endif  // FSEA_TUNE

}  // extern "C"
