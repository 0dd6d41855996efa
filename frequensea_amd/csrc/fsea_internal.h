// fsea_internal.h -- what the translation units of libfsea_hip.so share behind the C ABI (include/fsea.h): the plan
// object, error plumbing, the launch dispatcher, the owning types, and the scaffold of the thirteen device objects (FIR, IQ
// draw, demod, interp, chain, zoom, pfb, persist, cfar, events, trace, detect, capture).
//
// The owning types: a struct here releases HIP resources only by having members that release themselves.  Buffer<Mem>
// (memory that grows on demand), DeviceArray<T> and PinnedArray<T> (exact size, allocated once), Stream and Event, and
// Owned<T, destroy> (an inner object or plan, destroyed through its own C entry point).  No struct has a release list, so
// a failed create frees whatever it got as far as making, and the order of the members is the order of release, reversed.
//
// The scaffold: shared argument checks, create_object / destroy_object / reset_object, the event-ordered scratch buffer
// (SharedScratch), host-form staging (HostStaging).  A host form with several outputs (rows and pairs, two images and
// pairs) hands HostStaging::run its parts: they lie behind one another in the staging at 16-byte boundaries and come back
// in one copy and one wait.  The filter state of fsea_fir, fsea_zoom and fsea_pfb is FirState (fsea_fir_stage.h), whose
// tail length each object gives at create: FSEA_FIR_MAX_TAPS samples, or the bank's L - 1.  What fsea_persist, fsea_cfar
// and fsea_events share as consumers of rows of levels -- the head of their structs, the row checks, the packing of host
// rows, the zeroed accumulator -- is fsea_rows.h; what fsea_extract, fsea_measure and fsea_audio share as runners of a table of jobs
// -- the look-up on the device, the table's way there, the checks of a table -- is fsea_jobs.h.  What stays written out:
// fsea_plan_reset (it clears the counter slots too), fsea_interp_reset (nothing to zero and no second wait without
// elements), and the two device-wide waits of fsea_demod (before an evicted index table is released and before the
// stage-1 buffer grows).
//
// fsea_api.hip: the error plumbing, the scaffold's bodies and the entry points that take no plan;
// fsea_plan.hip: the kernel registry, a plan's life cycle, the launch path and the device-buffer entry points;
// fsea_plan_host.hip: the host-buffer entry points and the history ring; fsea_anysize.hip: the transform sizes without a
// kernel of their own (Bluestein's algorithm, four-step decomposition).
#pragma once

#include "../../include/fsea.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>

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

// A buffer that grows on demand and frees itself, one type per memory kind: device memory and default pinned host memory
// (the source and target of copies) with a quarter of headroom, mapped host memory (a kernel reads and writes it itself)
// with a 64 KiB floor and none.  grow(need): at least `need` bytes behind `ptr`, reallocated when `cap` is short.  The old
// memory is freed without any wait: a caller whose buffer work may still use waits for that work first.
// grow(need, keep), device memory on an idle device: the same, and the first `keep` bytes move along -- new memory, a
// device-to-device copy, then the old memory is freed; a failed copy frees the new memory and leaves the old in place.
enum class Mem { Device, Pinned, Mapped };
template <Mem K>
struct Buffer {
    void *ptr = nullptr;
    size_t cap = 0;

    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    ~Buffer() { if (ptr) (void)release(ptr); }
    static hipError_t alloc(void **p, size_t n) {
        return K == Mem::Device ? hipMalloc(p, n) : hipHostMalloc(p, n, K == Mem::Mapped ? hipHostMallocMapped : hipHostMallocDefault);
    }
    static hipError_t release(void *p) { return K == Mem::Device ? hipFree(p) : hipHostFree(p); }
    static size_t headroom(size_t need) { return K == Mem::Mapped ? (need < 65536 ? 65536 : need) : need + need / 4 + 4096; }
    int grow(size_t need) {
        if (cap >= need) return FSEA_OK;
        if (ptr) FSEA_HIP(release(ptr));
        ptr = nullptr;
        cap = 0;
        FSEA_HIP(alloc(&ptr, headroom(need)));
        cap = headroom(need);
        return FSEA_OK;
    }
    int grow(size_t need, size_t keep) {
        static_assert(K == Mem::Device, "the copy is device to device");
        if (cap >= need) return FSEA_OK;
        void *grown = nullptr, *old = ptr;
        FSEA_HIP(alloc(&grown, headroom(need)));
        const hipError_t e = keep ? hipMemcpy(grown, old, keep, hipMemcpyDeviceToDevice) : hipSuccess;
        if (e != hipSuccess) {
            (void)release(grown);
            return fail(FSEA_EHIP, "hipMemcpy failed: %s", hipGetErrorString(e));
        }
        ptr = grown;
        cap = headroom(need);
        if (old) FSEA_HIP(release(old));
        return FSEA_OK;
    }
};
using DeviceBuffer = Buffer<Mem::Device>;
using PinnedBuffer = Buffer<Mem::Pinned>;
using MappedBuffer = Buffer<Mem::Mapped>;

// `count` elements of device or default pinned memory, allocated once at exactly that size and freed with their owner;
// it moves, so a struct that holds one can live in a std::vector.  upload: allocate and copy from the host (nothing to
// allocate for a count of zero); zeros: allocate and zero; zero: zero again.  Those three are the device kind's.
template <class T, Mem K>
struct Array {
    T *ptr = nullptr;

    Array() = default;
    Array(Array &&o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    Array &operator=(Array &&o) noexcept {   // the old memory goes with `o`
        std::swap(ptr, o.ptr);
        return *this;
    }
    ~Array() { if (ptr) (void)Buffer<K>::release(ptr); }
    hipError_t alloc(size_t count) { return Buffer<K>::alloc(reinterpret_cast<void **>(&ptr), count * sizeof(T)); }
    hipError_t zero(size_t count) { return hipMemset(ptr, 0, count * sizeof(T)); }
    hipError_t zeros(size_t count) {
        const hipError_t e = alloc(count);
        return e == hipSuccess ? zero(count) : e;
    }
    template <class U>   // T itself, or the host's name for the same bytes (fsea::TwPair for fsea::cf)
    hipError_t upload(const U *host, size_t count) {
        static_assert(sizeof(U) == sizeof(T), "one host element per device element");
        if (!count) return hipSuccess;
        const hipError_t e = alloc(count);
        return e == hipSuccess ? hipMemcpy(ptr, host, count * sizeof(T), hipMemcpyHostToDevice) : e;
    }
};
template <class T>
using DeviceArray = Array<T, Mem::Device>;
template <class T>
using PinnedArray = Array<T, Mem::Pinned>;

// A non-blocking stream and an event, destroyed with their owner.  An event takes its flag when it is created: no timing
// unless hipEventDefault is asked for.  Both stand where the raw handle would.
struct Stream {
    hipStream_t s = nullptr;

    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;

    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// An inner object or plan, destroyed through its own C entry point (which brings the device, or the plan's stream, to rest
// first).  Declared after the memory and streams the inner object may use, so that it goes before them.
template <class T, int (*Destroy)(T *)>
struct Owned {
    T *ptr = nullptr;

    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { if (ptr) (void)Destroy(ptr); }
    T *operator->() const { return ptr; }
    operator T *() const { return ptr; }
};

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
    PinnedBuffer h_in, h_out;
    DeviceBuffer d_in, d_out;
    Stream stream;

    hipError_t create() { return stream.create(); }
    int reserve(size_t in_bytes, size_t out_bytes);

    // One output of a host-form call: `bytes` to `host`.  A part whose pointer is null or whose size is zero is not asked
    // for: it takes no room and its device address is null.
    struct Part {
        void *host;
        size_t bytes;
    };

    // One host-form call: fill(h_in) writes the in_bytes of input into pinned memory, copy in, launch(d_in, d_parts, stream)
    // queues the object's work, copy out, wait, every part to its host pointer.  The parts lie behind d_out / h_out in
    // their order, each at a 16-byte boundary; d_parts[i] is the device address of part i.  A launch may put memory of
    // the object's own there instead: that part comes back in a copy of its own, queued behind the one copy of all that
    // is staged.  Zero-byte copies are skipped.  The caller holds the object's mutex and is on its device.  With a
    // `deliver`, deliver(i, h) takes part i from pinned memory in place of the copy of the whole part to its host pointer.
    template <size_t N, class Fill, class Launch, class Deliver>
    int run(size_t in_bytes, const Part (&parts)[N], Fill &&fill, Launch &&launch, Deliver &&deliver) {
        size_t at[N], bytes[N], end = 0;
        for (size_t i = 0; i < N; ++i) {
            bytes[i] = parts[i].host ? parts[i].bytes : 0;
            at[i] = (end + 15) & ~(size_t)15;
            if (bytes[i]) end = at[i] + bytes[i];
        }
        int rc = reserve(in_bytes, end);
        if (rc) return rc;
        if (in_bytes) {
            fill(h_in.ptr);
            FSEA_HIP(hipMemcpyAsync(d_in.ptr, h_in.ptr, in_bytes, hipMemcpyHostToDevice, stream));
        }
        uint8_t *h = static_cast<uint8_t *>(h_out.ptr), *d = static_cast<uint8_t *>(d_out.ptr);
        void *d_parts[N];
        for (size_t i = 0; i < N; ++i) d_parts[i] = bytes[i] ? d + at[i] : nullptr;
        rc = launch(d_in.ptr, d_parts, stream);
        if (rc) return rc;
        size_t staged = 0;
        for (size_t i = 0; i < N; ++i) {
            if (bytes[i] && d_parts[i] == d + at[i]) staged = at[i] + bytes[i];
        }
        if (staged) FSEA_HIP(hipMemcpyAsync(h, d, staged, hipMemcpyDeviceToHost, stream));
        for (size_t i = 0; i < N; ++i) {
            if (bytes[i] && d_parts[i] != d + at[i]) {
                FSEA_HIP(hipMemcpyAsync(h + at[i], d_parts[i], bytes[i], hipMemcpyDeviceToHost, stream));
            }
        }
        FSEA_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < N; ++i) {
            if (bytes[i]) deliver(i, static_cast<const uint8_t *>(h + at[i]));
        }
        return FSEA_OK;
    }
    template <size_t N, class Fill, class Launch>
    int run(size_t in_bytes, const Part (&parts)[N], Fill &&fill, Launch &&launch) {
        return run(in_bytes, parts, fill, launch, [&](size_t i, const uint8_t *h) { std::memcpy(parts[i].host, h, parts[i].bytes); });
    }

    // the same with one output: launch(d_in, d_out, stream)
    template <class Fill, class Launch>
    int run(size_t in_bytes, size_t out_bytes, void *out, Fill &&fill, Launch &&launch) {
        const Part part[1] = {{out, out_bytes}};
        return run(in_bytes, part, fill, [&](void *d_in, void **d_parts, hipStream_t s) { return launch(d_in, d_parts[0], s); });
    }
};

// A growable device buffer that an object's launches use on whatever stream the caller names.  One event keeps them in
// order: acquire(s) makes s wait for the previous use, release(s) records the end of this one, and reserve() waits on the
// host for the last use before the buffer is reallocated (or, by the caller, overwritten).  acquire(need, s) is how a
// launch begins: reserve(need) where the buffer is shorter than that, then acquire(s).  The caller holds the object's
// mutex and is on its device.
struct SharedScratch {
    DeviceBuffer buf;
    Event used;  // recorded after the last work that used the buffer

    hipError_t create(hipStream_t first);  // the event starts recorded on `first`, so it can be waited for at once
    int reserve(size_t need);
    int acquire(hipStream_t s);
    int acquire(size_t need, hipStream_t s);
    int release(hipStream_t s);
};

// FSEA_OK, or FSEA_EHIP with "<what>: <HIP's text>"; an int code passes through (what an object's initialiser returns)
int init_code(const char *what, hipError_t e);
inline int init_code(const char *, int rc) { return rc; }

// What every fsea_X_create does once its own arguments are checked: device check, `new`, the staging stream, then
// init(obj) -> hipError_t or an FSEA_* code, on the object's device.  T has `device` and `staging`; its members free
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

// fsea_X_reset: `null_message` for a NULL object; under the object's mutex and on its device, body() -> FSEA_* code zeroes
// the state between two waits for the device (launches on any stream may use the state; the zeroes are in place before
// the next one)
template <class T, class Body>
int reset_object(T *obj, const char *null_message, Body &&body) {
    if (!obj) return fail(FSEA_EINVAL, "%s", null_message);
    std::lock_guard<std::mutex> lock(obj->mu);
    FSEA_ON_DEVICE(obj->device);
    FSEA_HIP(hipDeviceSynchronize());
    if (int rc = body()) return rc;
    FSEA_HIP(hipDeviceSynchronize());
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

// A plan is made of parts that own what they hold (the owning types above), so fsea_plan_destroy is a `delete` and a failed
// fsea_plan_create frees whatever it got as far as allocating.
struct fsea_plan {
    int n = 0;
    int hop = 0;
    int mode = 0;
    int device = 0;
    const fsea::KernelEntry *entry = nullptr;
    fsea_detail::DeviceArray<fsea::cf> d_tw;  // passes 1..np-1 concatenated
    size_t tw_off[5] = {0, 0, 0, 0, 0};  // passes 0..3, then the HI/LO factor tables (fsea_tables.h)
    size_t tw_def_off = 0;               // deferred middle-pass table (fo::DEFER / fo::V2), 16-byte aligned
    int num_cu = 0;
    fsea_detail::DeviceArray<unsigned long long> d_trace;  // FSEA_TRACE diagnostics (tuning library)
    int occ[fsea::K_COUNT] = {};
    // FSEA_UNITS_AUTO: launches with at most FSEA_STATIC_UNITS_PER_WG units per workgroup use the static interleave,
    // longer ones the ticket pools; fsea_plan_set_unit_distribution pins one of the two
    int units_policy = FSEA_UNITS_AUTO;
    int half_run_max = 32;         // frames per run of the half-overlap kernels at most (FSEA_HALF_RUN_MAX at plan creation; 8, 16 and 32 equal in rate, fetch 1.127x / 1.064x / 1.033x the distinct bytes: profiles/r04_stft_run_length.txt)
    bool no_half_overlap = false;  // FSEA_NO_HALF_OVERLAP=1 at plan creation: hop == N/2 runs the ordinary kernel (A/B measurements)

    // Ticket counters of the multi-wave sizes: one slot per stream the plan is launched on.  Launches
    // on one stream run in order and the last workgroup of a launch zeroes its slot, so a stream
    // needs exactly one; launches on different streams may overlap and never share one.
    struct Counters {
        fsea_detail::DeviceArray<unsigned> d_ctr;  // FSEA_CTR_SLOTS x FSEA_CTR_WORDS
        std::mutex slot_mu;
        struct Slot {
            hipStream_t stream = nullptr;   // the stream the slot serves (meaningful while `used` and not `anonymous`)
            fsea_detail::Event ev;          // recorded behind the slot's last launch (not while the stream is being captured); created on first use
            bool used = false, pending = false, anonymous = false, captured = false;
            bool launching = false;         // claimed by a host thread between counter_slot() and the record of `ev`: not to be recycled
            unsigned long long seq = 0;     // launch order, for least-recently-used recycling
        } slots[FSEA_CTR_SLOTS];
        unsigned long long slot_seq = 0;

        hipError_t create();  // the counters, zeroed on the null stream: the caller waits for the device before a launch
    } ctr;

    // The host-buffer entry points (fsea_plan_host.hip), one call at a time under `mu`.
    struct HostPath {
        std::mutex mu;
        // device staging of the large batches; d_aux also holds the rows that fsea_mean_magnitude_u8_device sums into d_acc
        fsea_detail::DeviceBuffer d_in, d_out, d_aux;
        fsea_detail::DeviceArray<double> d_acc;
        // small host batches (the nrf_fft_process pattern: one 2 KiB frame in, one row out) go through
        // pinned, device-mapped staging: the kernel reads and writes host memory itself, so a call is
        // one launch and one synchronisation instead of copy + launch + copy
        fsea_detail::MappedBuffer h_in, h_out;
        // the pipelined host-buffer path (exec_host_pipelined): copy-in and copy-out streams beside the plan's stream, and
        // one "chunk arrived" / "chunk transformed" event pair per chunk in flight
        fsea_detail::Stream s_h2d, s_d2h;
        fsea_detail::Event ev_in[FSEA_HOST_CHUNKS_MAX], ev_done[FSEA_HOST_CHUNKS_MAX];

        hipError_t create();  // the two streams and the events

        // One small batch through the mapped staging: fill(h_in) writes the in_bytes of input, launch(d_in, d_out) queues the
        // transform on `stream` with the staging's device addresses, wait, out_bytes to `out`.  `out` null: the launch writes
        // device memory of its own, no output staging.  The caller holds `mu` and is on the plan's device.
        template <class Fill, class Launch>
        int zero_copy(hipStream_t stream, size_t in_bytes, size_t out_bytes, void *out, Fill &&fill, Launch &&launch) {
            int rc = h_in.grow(in_bytes);
            if (!rc && out) rc = h_out.grow(out_bytes);
            if (rc) return rc;
            void *d_src = nullptr, *d_dst = nullptr;
            FSEA_HIP(hipHostGetDevicePointer(&d_src, h_in.ptr, 0));
            if (out) FSEA_HIP(hipHostGetDevicePointer(&d_dst, h_out.ptr, 0));
            fill(h_in.ptr);
            rc = launch(d_src, d_dst);
            if (rc) return rc;
            FSEA_HIP(hipStreamSynchronize(stream));
            if (out) std::memcpy(out, h_out.ptr, out_bytes);
            return FSEA_OK;
        }
    } host;

    // Bluestein plans (transform sizes without a kernel of their own): `n` is the logical size, `entry` the power-of-two
    // kernel set of size blu.m the convolution runs on
    struct Bluestein {
        int m = 0;
        fsea_detail::DeviceArray<fsea::cf> chirp;   // conj(w[j]), j < n
        fsea_detail::DeviceArray<fsea::cf> bfft;    // FFT_m of the wrapped chirp
        fsea_detail::DeviceArray<fsea::cf> dc;      // spectrum of the offset-binary DC term, n entries
        fsea_detail::Owned<fsea_plan, fsea_plan_destroy> inner;   // size m, COMPLEX_F32; the first to go
    } blu;

    // four-step plans (powers of two above 16384): n = fs.n1 * fs.n2, two inner plans, the twiddles W_n^{j2 k1}
    struct FourStep {
        int n1 = 0, n2 = 0;
        fsea_detail::DeviceArray<fsea::cf> tw;
        fsea_detail::Owned<fsea_plan, fsea_plan_destroy> inner2, inner1;   // inner1 goes first, then inner2, then tw
    } fs;

    // What a Bluestein and a four-step plan share: two work buffers of `frames` frames each.  They are the plan's, not the
    // launch's: launches of such a plan on different streams are put in order behind one another (an event recorded
    // behind each launch, waited for by the next one's stream)
    struct Work {
        fsea_detail::DeviceArray<fsea::cf> buf[2];
        size_t frames = 0;
        std::mutex mu;
        fsea_detail::Event ev;   // created by the first launch
        bool pending = false;
    } work;

    // taper window (fsea_plan_set_window): weights in the pass-0 lane order with (-1)^n folded in, and the DC term's
    // spectrum around bin n/2 (FftArgs::win, win_dc); form 0 = none, 1 = centred, 2 = offset-binary
    struct Window {
        fsea_detail::DeviceArray<float> d_win;
        fsea_detail::DeviceArray<fsea::cf> d_win_dc;
        int form = 0;
    } window;

    // both strings live as long as the plan: fsea_plan_kernel_name hands out a pointer into the one in use, and a pointer a
    // caller got earlier stays valid across fsea_plan_set_window (the windowed name depends on the plan's constants only)
    std::string kernel_name;        // while no window is set
    std::string kernel_name_win;    // while one is (filled by the first fsea_plan_set_window)

    // the last members, so the first to be released: the plan's own stream (fsea_plan_destroy has waited for it), and the
    // events around the launches fsea_time_exec_* time (tuning library; created by every build)
    fsea_detail::Stream stream;
    fsea_detail::Event ev0, ev1;
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
