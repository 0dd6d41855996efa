// fsea_internal.h -- what the translation units of libfsea_hip.so share behind the C ABI (include/fsea.h): the plan
// object, error plumbing, the launch dispatcher, and the scaffold of the six device objects (FIR, IQ draw, demod, interp,
// chain, trace): shared argument checks, create / destroy, growable buffers, the event-ordered scratch buffer, host-form
// staging.  fsea_api.hip: plans, the power-of-two launches, every entry point, the scaffold's bodies;
// fsea_anysize.hip: the transform sizes without a kernel of their own (Bluestein's algorithm, four-step decomposition).
#pragma once

#include "../../include/fsea.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <new>
#include <string>

#include "fsea_registry.h"

#define FSEA_STATIC_UNITS_PER_WG 16u  // measured crossover: profiles/r02_static_vs_ticket_distribution.txt
#define FSEA_CTR_SLOTS 64u          // ticket-counter slots = streams one plan may be launched on concurrently
#define FSEA_HOST_CHUNKS_MAX 16      // chunks of one host-buffer call (fsea_exec_*_host) in flight
#define FSEA_CTR_WORDS (9u * 32u + 2048u)  // 8 ticket pools + the finished-workgroups word, one 128-byte line each; one progress word per workgroup (tuning option)


namespace fsea_detail {

int fail(int code, const char *fmt, ...);
size_t mode_elem_bytes(int mode);

#define FSEA_HIP(call)                                                                            \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            return fsea_detail::fail(FSEA_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                \
        }                                                                                         \
    } while (0)


// Every entry point works on the plan's device and leaves the caller's current device as it was
// (a host process driving several GPUs, torch included, keeps its own notion of "current").
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
        else prev = -1;  // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define FSEA_ON_DEVICE(dev)                                                                       \
    DeviceGuard device_guard_(dev);                                                               \
    if (device_guard_.err != hipSuccess) {                                                        \
        return fsea_detail::fail(FSEA_EHIP, "hipSetDevice(%d) failed: %s", (dev), hipGetErrorString(device_guard_.err)); \
    }

// where the rows of a launch go when they are tiles of an image (fsea_exec_u8_tiled_device); rows == 0: contiguous
struct TileLayout {
    uint32_t rows = 0, pitch_row = 0, pitch_tile = 0;
    size_t span = 0;
};

// x86-64's (uint8_t)(v * 256.0), the reference's nut_buffer_set_f64 / nut_buffer_get_u8 on a u8 buffer: truncate to int32,
// 0x80000000 outside its range or for NaN, keep the low byte.  AMDGPU's v_cvt_i32_f64 saturates instead, so the range
// check is explicit.
__device__ __forceinline__ uint32_t coord_f64(double v) {
    const double s = v * 256.0;
    if (!(s > -2147483649.0 && s < 2147483648.0)) return 0u;
    return (uint32_t)(int)s & 0xffu;
}

// At least `need` bytes in *ptr (device memory, or pinned host memory), reallocated with headroom when *cap is short.  The
// old buffer is freed without any wait: a caller whose buffer work may still use waits for that work first.
int grow_device(void **ptr, size_t *cap, size_t need);
int grow_pinned(void **ptr, size_t *cap, size_t need);

// FSEA_OK, FSEA_ENODEVICE when HIP has no device at all, FSEA_EINVAL when `device` is not one of them
int check_device(int device);

// Argument checks that several objects share, with the one message each has.  `names` is what the caller's message says
// must be 16-byte aligned ("d_iq and d_out", "the outputs", ...).
int check_multiplier(int size_multiplier);
int check_n_frames(int n_frames);
int check_aligned16(const char *names, const void *a, const void *b = nullptr, const void *c = nullptr);

// The host-buffer forms of a device object: its own non-blocking stream and pinned + device staging, grown on demand.
// Only those forms use the staging, on that stream, under the object's mutex.
struct HostStaging {
    hipStream_t stream = nullptr;
    void *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
    size_t h_in_bytes = 0, h_out_bytes = 0, d_in_bytes = 0, d_out_bytes = 0;

    hipError_t create() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
    ~HostStaging();
    int reserve(size_t in_bytes, size_t out_bytes);

    // One host-form call: fill(h_in) writes the in_bytes of input into pinned memory, copy in, launch(d_in, d_out, stream)
    // queues the object's work, copy out, wait, out_bytes to `out`.  Zero-byte copies are skipped.  The caller holds the
    // object's mutex and is on its device.
    template <class Fill, class Launch>
    int run(size_t in_bytes, size_t out_bytes, void *out, Fill &&fill, Launch &&launch) {
        int rc = reserve(in_bytes, out_bytes);
        if (rc) return rc;
        if (in_bytes) {
            fill(h_in);
            FSEA_HIP(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, stream));
        }
        rc = launch(d_in, d_out, stream);
        if (rc) return rc;
        if (out_bytes) FSEA_HIP(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, stream));
        FSEA_HIP(hipStreamSynchronize(stream));
        if (out_bytes) std::memcpy(out, h_out, out_bytes);
        return FSEA_OK;
    }
};

// A growable device buffer that an object's launches use on whatever stream the caller names.  One event keeps them in
// order: acquire(s) makes s wait for the previous use, release(s) records the end of this one, and reserve() waits on the
// host for the last use before the buffer is reallocated (or, by the caller, overwritten).  The caller holds the object's
// mutex and is on its device.
struct SharedScratch {
    void *ptr = nullptr;
    size_t bytes = 0;
    hipEvent_t used = nullptr;  // recorded after the last work that used the buffer

    hipError_t create(hipStream_t first);  // the event starts recorded on `first`, so it can be waited for at once
    ~SharedScratch();
    int reserve(size_t need);
    int acquire(hipStream_t s);
    int release(hipStream_t s);
};

// FSEA_OK, or FSEA_EHIP with "<what>: <HIP's text>"; an int code passes through (what an object's initialiser returns)
int init_code(const char *what, hipError_t e);
inline int init_code(const char *, int rc) { return rc; }

// What every fsea_X_create does once its own arguments are checked: device check, `new`, the staging stream, then
// init(obj) -> hipError_t or an FSEA_* code, on the object's device.  T has `device`, `staging` and a destructor that frees
// whatever init got as far as allocating.  `what` is the entry point's name, for the failure text.
template <class T, class Init>
int create_object(T **out, int device, const char *what, Init &&init) {
    int rc = check_device(device);
    if (rc) return rc;
    FSEA_ON_DEVICE(device);
    T *obj = new (std::nothrow) T();
    if (!obj) return fail(FSEA_ENOMEM, "out of host memory");
    obj->device = device;
    rc = init_code(what, obj->staging.create());
    if (!rc) rc = init_code(what, init(obj));
    if (rc) {
        delete obj;
        return rc;
    }
    *out = obj;
    return FSEA_OK;
}

// fsea_X_destroy: NULL is fine; launches of the object on any stream may still use what it owns, so the device is idle
// before the destructor frees it
template <class T>
int destroy_object(T *obj) {
    if (!obj) return FSEA_OK;
    FSEA_ON_DEVICE(obj->device);
    FSEA_HIP(hipDeviceSynchronize());
    delete obj;
    return FSEA_OK;
}

// The frequency shift of fsea_fir_u8_shifted_* (include/fsea.h).
struct FirShift {
    double cycles_per_sample, phase0_cycles;
    uint64_t sample_offset;
};

// One launch of a FIR object on device buffers, asynchronous on `s`, arguments checked first: n_in samples of 8-bit
// (f64 == 0) or f64 IQ behind d_in, shifted when `shift` is not null, followed by n_zero samples of plain 0.0 (only with a
// shift: the back half of nrf_freq_shifter's buffer); n_in + n_zero pairs to d_out.  What fsea_fir_u8_device and
// fsea_fir_u8_shifted_device call, and fsea_chain for the forms the C ABI has no name for.
int fir_launch_device(fsea_fir *f, int f64, const void *d_in, size_t n_in, size_t n_zero, int flip, const FirShift *shift,
                      void *d_out, hipStream_t s);

}  // namespace fsea_detail

struct fsea_plan {
    int n = 0;
    int hop = 0;
    int mode = 0;
    int device = 0;
    const fsea::KernelEntry *entry = nullptr;
    hipStream_t stream = nullptr;
    fsea::cf *d_tw = nullptr;      // passes 1..np-1 concatenated
    size_t tw_off[5] = {0, 0, 0, 0, 0};  // passes 0..3, then the HI/LO factor tables (fsea_tables.h)
    size_t tw_def_off = 0;               // deferred middle-pass table (fo::DEFER / fo::V2), 16-byte aligned
    int num_cu = 0;
    // Ticket counters of the multi-wave sizes: one slot per stream the plan is launched on.  Launches
    // on one stream run in order and the last workgroup of a launch zeroes its slot, so a stream
    // needs exactly one; launches on different streams may overlap and never share one.
    unsigned *d_ctr = nullptr;  // FSEA_CTR_SLOTS x FSEA_CTR_WORDS
    std::mutex slot_mu;
    struct CtrSlot {
        hipStream_t stream = nullptr;   // the stream the slot serves (meaningful while `used` and not `anonymous`)
        hipEvent_t ev = nullptr;        // recorded behind the slot's last launch (not while the stream is being captured)
        bool used = false, pending = false, anonymous = false, captured = false;
        bool launching = false;         // claimed by a host thread between counter_slot() and the record of `ev`: not to be recycled
        unsigned long long seq = 0;     // launch order, for least-recently-used recycling
    } slots[FSEA_CTR_SLOTS];
    unsigned long long slot_seq = 0;
    unsigned long long *d_trace = nullptr;  // FSEA_TRACE diagnostics (tuning library)
    int occ[fsea::K_COUNT] = {};
    // FSEA_UNITS_AUTO: launches with at most FSEA_STATIC_UNITS_PER_WG units per workgroup use the static interleave,
    // longer ones the ticket pools; fsea_plan_set_unit_distribution pins one of the two
    int units_policy = FSEA_UNITS_AUTO;
    int half_run_max = 32;         // frames per run of the half-overlap kernels at most (FSEA_HALF_RUN_MAX at plan creation; 8, 16 and 32 equal in rate, fetch 1.127x / 1.064x / 1.033x the distinct bytes: profiles/r04_stft_run_length.txt)
    bool no_half_overlap = false;  // FSEA_NO_HALF_OVERLAP=1 at plan creation: hop == N/2 runs the ordinary kernel (A/B measurements)
    // staging for the host-buffer entry points
    std::mutex mu;
    void *d_in = nullptr;
    size_t d_in_bytes = 0;
    void *d_out = nullptr;
    size_t d_out_bytes = 0;
    void *d_aux = nullptr;
    size_t d_aux_bytes = 0;
    double *d_acc = nullptr;
    // small host batches (the nrf_fft_process pattern: one 2 KiB frame in, one row out) go through
    // pinned, device-mapped staging: the kernel reads and writes host memory itself, so a call is
    // one launch and one synchronisation instead of copy + launch + copy
    void *h_in = nullptr;
    void *h_out = nullptr;
    size_t h_in_bytes = 0, h_out_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the pipelined host-buffer path (exec_host_pipelined): copy-in and copy-out streams beside `stream`, and one
    // "chunk arrived" / "chunk transformed" event pair per chunk in flight
    // Bluestein plans (transform sizes without a kernel of their own): `n` is the logical size, `entry` the power-of-two
    // kernel set of size blu_m the convolution runs on
    int blu_m = 0;
    fsea_plan *blu_inner = nullptr;          // size blu_m, COMPLEX_F32
    fsea::cf *d_blu_chirp = nullptr;         // conj(w[j]), j < n
    fsea::cf *d_blu_bfft = nullptr;          // FFT_m of the wrapped chirp
    fsea::cf *d_blu_dc = nullptr;            // spectrum of the offset-binary DC term, n entries
    fsea::cf *d_blu_work[2] = {nullptr, nullptr};
    size_t blu_work_frames = 0;
    // the work buffers are the plan's, not the launch's: launches of such a plan on different streams are put in order
    // behind one another (an event recorded behind each launch, waited for by the next one's stream)
    std::mutex work_mu;
    hipEvent_t work_ev = nullptr;
    bool work_pending = false;
    // four-step plans (powers of two above 16384): n = fs_n1 * fs_n2, two inner plans, the twiddles W_n^{j2 k1}
    int fs_n1 = 0, fs_n2 = 0;
    fsea_plan *fs_inner1 = nullptr, *fs_inner2 = nullptr;
    fsea::cf *d_fs_tw = nullptr;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_in[FSEA_HOST_CHUNKS_MAX] = {}, ev_done[FSEA_HOST_CHUNKS_MAX] = {};
    // taper window (fsea_plan_set_window): weights in the pass-0 lane order with (-1)^n folded in, and the DC term's
    // spectrum around bin n/2 (FftArgs::win, win_dc); window_form 0 = none, 1 = centred, 2 = offset-binary
    float *d_win = nullptr;
    fsea::cf *d_win_dc = nullptr;
    int window_form = 0;
    // both strings live as long as the plan: fsea_plan_kernel_name hands out a pointer into the one in use, and a pointer a
    // caller got earlier stays valid across fsea_plan_set_window (the windowed name depends on the plan's constants only)
    std::string kernel_name;        // while no window is set
    std::string kernel_name_win;    // while one is (filled by the first fsea_plan_set_window)
};


namespace fsea_detail {

// One batch of frames through whatever serves the plan's size: a power-of-two kernel, Bluestein's algorithm, or the
// four-step decomposition (the latter two call back into this for their inner transforms).
int launch(fsea_plan *p, int in_kind, const void *d_in, size_t n_frames, int flip, int mode, void *d_out, hipStream_t s,
           double rot_delta = 0.0, double rot_phase0 = 0.0, const TileLayout *tiles = nullptr);

// fsea_anysize.hip
#define FSEA_MAX_FFT_SIZE (1 << 20)  // largest transform: four-step up to 2^20 points; Bluestein's m = 2^p >= 2n - 1 within it
bool fourstep_split(int n, int *n1, int *n2);
int bluestein_m(int n);
int blu_setup(fsea_plan *p);
int fs_setup(fsea_plan *p);
int blu_launch(fsea_plan *p, int in_kind, const void *d_in, size_t n_frames, int flip, int mode, void *d_out, hipStream_t s);
int fs_launch(fsea_plan *p, int in_kind, const void *d_in, size_t n_frames, int flip, int mode, void *d_out, hipStream_t s);

}  // namespace fsea_detail
