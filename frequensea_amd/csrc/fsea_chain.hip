// fsea_chain.hip -- the per-block chain of the reference's IQ scenes (include/fsea.h: fsea_chain_*): optional frequency
// shift -> low-pass filter -> constellation images (lua/dvbt.lua:46-51, lua/iq-tex-filtered.lua:44-47), with the filtered
// block resident on the device between the steps.
//
// No kernel lives here.  A run queues, on one stream: the upload of the 8-bit block, one filter launch into the object's
// buffer of f32 pairs (fsea_fir_u8 or fsea_shift_fir_u8 through fsea_detail::fir_launch_device), the draw launches that read
// that buffer as FSEA_IQ_F32 (fsea_iq_points_device / fsea_iq_lines_device), the downloads of what was asked for, and
// waits once.  The block sequence it replaces moves the filtered block to the host as f32, widens it to f64 there and
// uploads it again for every image.
#include "fsea_fir_stage.h"

#include <cstring>

using fsea_detail::DeviceGuard;
using fsea_detail::fail;
using fsea_detail::FirShift;

struct fsea_chain {
    int device = 0;
    fsea_detail::DeviceBuffer pairs;  // the filtered (I, Q) f32 pairs of the last run, frame after frame
    size_t n_pairs = 0;       // pairs per frame of the resident block
    std::mutex mu;
    fsea_detail::HostStaging staging;  // the host forms: input, images and their pinned twins
    // the inner objects are the first to go: the filter, then the drawer
    fsea_detail::Owned<fsea_iq_draw, fsea_iq_draw_destroy> draw;
    fsea_detail::Owned<fsea_fir, fsea_fir_destroy> fir;
};

namespace {

constexpr size_t IMAGE_BYTES = 65536;            // a points image
constexpr size_t MAX_PAIRS = (size_t)1 << 31;    // per frame, as the draw functions
constexpr size_t MAX_TOTAL = (size_t)1 << 40;

const fsea_chain_stage NO_STAGE = {0, 0, 0.0, 0.0, 0, 0};
const fsea_chain_outputs NO_OUTPUTS = {nullptr, nullptr, 1, 0, nullptr};

size_t line_pixels(const fsea_chain_outputs &o) { return o.lines ? IMAGE_BYTES * o.size_multiplier * o.size_multiplier : 0; }

int check_stage(const fsea_chain_stage &st, size_t n, int n_frames) {
    if (int rc = fsea_detail::check_n_frames(n_frames)) return rc;
    if (st.n_zero && !st.shift) return fail(FSEA_EINVAL, "n_zero needs a frequency shift");
    if (n > MAX_PAIRS || st.n_zero > MAX_PAIRS || n + st.n_zero > MAX_PAIRS ||
        (n_frames && n + st.n_zero > MAX_TOTAL / (size_t)n_frames)) {
        return fail(FSEA_EINVAL, "%zu + %zu pairs x %d frames is too large", n, st.n_zero, n_frames);
    }
    if (n_frames > 1 && st.n_zero && ((n & 7) || (st.n_zero & 1))) {
        return fail(FSEA_EINVAL, "frames with zero samples need n_samples a multiple of 8 and n_zero even");
    }
    // the shift of the whole call, here and not piece by piece: the frames stand at sample_offset + f n (the zeros are not
    // the shifter's samples), so no launch of queue_filter can be refused once an earlier one is queued.  Without a shift
    // the three fields are not looked at.
    if (st.shift) {
        const size_t span = n * (size_t)(n_frames > 0 ? n_frames : 0);   // <= MAX_TOTAL: checked above
        return fsea_stage::check_shift(st.cycles_per_sample, st.phase0_cycles, st.sample_offset, span);
    }
    return FSEA_OK;
}

int check_outputs(const fsea_chain_outputs &o, size_t n_pairs, int n_frames, bool device) {
    if (o.lines) {
        if (int rc = fsea_detail::check_multiplier(o.size_multiplier)) return rc;
        if (o.n_line_points > n_pairs) {
            return fail(FSEA_EINVAL, "n_line_points %zu exceeds the %zu pairs of a frame", o.n_line_points, n_pairs);
        }
        if (n_frames > 1 && o.n_line_points != n_pairs && (n_pairs & 1)) {
            return fail(FSEA_EINVAL, "lines over a part of each frame need an even number of pairs per frame");
        }
    }
    return device ? fsea_detail::check_aligned16("the outputs", o.points, o.lines, o.pairs) : (int)FSEA_OK;
}

// the caller holds c->mu and is on c's device; stream work that may still read the old buffer is the caller's to order.
// The resident block goes only where the buffer has to be reallocated; otherwise it stays until a filter launch is queued.
int reserve_pairs(fsea_chain *c, size_t bytes) {
    const size_t need = bytes ? bytes : 16;
    if (c->pairs.cap < need) c->n_pairs = 0;
    return c->pairs.grow(need);
}

// the filter launches of n_frames blocks into c->pairs.ptr
int queue_filter(fsea_chain *c, int f64, const void *d_in, size_t n, int n_frames, const fsea_chain_stage &st, hipStream_t s) {
    FirShift shift = {st.cycles_per_sample, st.phase0_cycles, st.sample_offset};
    if (!st.n_zero) {   // the blocks are one piece of the stream: one launch
        return fsea_detail::fir_launch_device(c->fir, f64, d_in, n * (size_t)n_frames, 0, st.flip, st.shift ? &shift : nullptr,
                                              c->pairs.ptr, s);
    }
    for (int f = 0; f < n_frames; ++f) {
        shift.sample_offset = st.sample_offset + (uint64_t)f * n;   // the zeros are not the shifter's samples
        int rc = fsea_detail::fir_launch_device(c->fir, 0, static_cast<const uint8_t *>(d_in) + 2 * n * f, n, st.n_zero, st.flip,
                                                &shift, static_cast<float *>(c->pairs.ptr) + 2 * (n + st.n_zero) * f, s);
        if (rc) return rc;
    }
    return FSEA_OK;
}

// the draws of the resident frames into device images
int queue_images(fsea_chain *c, int n_frames, const fsea_chain_outputs &o, void *d_points, void *d_lines, hipStream_t s) {
    const size_t n = c->n_pairs;
    if (o.points) {
        int rc = fsea_iq_points_device(c->draw, c->pairs.ptr, FSEA_IQ_F32, 0, n, n_frames, d_points, s);
        if (rc) return rc;
    }
    if (o.lines) {
        if (o.n_line_points == n || n_frames <= 1) {
            return fsea_iq_lines_device(c->draw, c->pairs.ptr, FSEA_IQ_F32, 0, o.n_line_points, n_frames, o.size_multiplier,
                                        d_lines, s);
        }
        for (int f = 0; f < n_frames; ++f) {   // the frames' first points are not consecutive in the buffer
            int rc = fsea_iq_lines_device(c->draw, static_cast<const float *>(c->pairs.ptr) + 2 * n * f, FSEA_IQ_F32, 0,
                                          o.n_line_points, 1, o.size_multiplier,
                                          static_cast<uint8_t *>(d_lines) + line_pixels(o) * f, s);
            if (rc) return rc;
        }
    }
    return FSEA_OK;
}

// One host call: upload and filter n samples (run), then the outputs of the resident block: the images through the
// staging, the pairs straight from c->pairs.  The caller holds c->mu.
int host_call(fsea_chain *c, bool run, const void *in, int f64, size_t n, const fsea_chain_stage &st,
              const fsea_chain_outputs &o) {
    FSEA_ON_DEVICE(c->device);
    const size_t in_bytes = run ? n * (f64 ? 16 : 2) : 0;
    const size_t total = run ? n + st.n_zero : c->n_pairs;
    if (run) {
        if (int rc = reserve_pairs(c, total * 8)) return rc;
    }
    const fsea_detail::HostStaging::Part parts[3] = {{o.points, IMAGE_BYTES}, {o.lines, line_pixels(o)}, {o.pairs, total * 8}};
    return c->staging.run(
        in_bytes, parts, [&](void *h_in) { std::memcpy(h_in, in, in_bytes); },
        [&](void *d_in, void **d_parts, hipStream_t s) {
            if (run) {
                c->n_pairs = 0;   // from here on the buffer is being overwritten
                if (int rc = queue_filter(c, f64, d_in, n, 1, st, s)) return rc;
                c->n_pairs = total;
            }
            if (d_parts[2]) d_parts[2] = c->pairs.ptr;
            return queue_images(c, 1, o, d_parts[0], d_parts[1], s);
        });
}

int run_host(fsea_chain *c, const void *iq, int f64, size_t n, const fsea_chain_stage *stage, const fsea_chain_outputs *outputs) {
    if (!c) return fail(FSEA_EINVAL, "chain is NULL");
    const fsea_chain_stage &st = stage ? *stage : NO_STAGE;
    const fsea_chain_outputs &o = outputs ? *outputs : NO_OUTPUTS;
    if (n && !iq) return fail(FSEA_EINVAL, "NULL buffer");
    int rc = check_stage(st, n, 1);
    if (!rc) rc = check_outputs(o, n + st.n_zero, 1, false);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    return host_call(c, true, iq, f64, n, st, o);
}

}  // namespace

extern "C" {

int fsea_chain_create(fsea_chain **out, const double *taps, int n_taps, int device) {
    if (!out) return fail(FSEA_EINVAL, "chain out-pointer is NULL");
    *out = nullptr;
    if (int rc = fsea_stage::FirState::check_taps(taps, n_taps)) return rc;   // bad taps are reported before a missing device
    return fsea_detail::create_object(out, device, "fsea_chain_create", [&](fsea_chain *c) -> int {
        int rc = fsea_fir_create(&c->fir.ptr, taps, n_taps, device);
        return rc ? rc : fsea_iq_draw_create(&c->draw.ptr, device);
    });
}

int fsea_chain_destroy(fsea_chain *c) { return fsea_detail::destroy_object(c); }

int fsea_chain_reset(fsea_chain *c) {
    if (!c) return fail(FSEA_EINVAL, "chain is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    return fsea_fir_reset(c->fir);
}

size_t fsea_chain_n_pairs(const fsea_chain *c) { return c ? c->n_pairs : 0; }

int fsea_chain_run_host(fsea_chain *c, const uint8_t *iq, size_t n_samples, const fsea_chain_stage *stage,
                        const fsea_chain_outputs *outputs) {
    return run_host(c, iq, 0, n_samples, stage, outputs);
}

int fsea_chain_run_f64_host(fsea_chain *c, const double *iq, size_t n_samples, const fsea_chain_outputs *outputs) {
    return run_host(c, iq, 1, n_samples, nullptr, outputs);
}

int fsea_chain_fetch_host(fsea_chain *c, const fsea_chain_outputs *outputs) {
    if (!c) return fail(FSEA_EINVAL, "chain is NULL");
    const fsea_chain_outputs &o = outputs ? *outputs : NO_OUTPUTS;
    std::lock_guard<std::mutex> lock(c->mu);
    int rc = check_outputs(o, c->n_pairs, 1, false);
    if (rc) return rc;
    return host_call(c, false, nullptr, 0, 0, NO_STAGE, o);
}

int fsea_chain_run_device(fsea_chain *c, const void *d_iq, size_t n_samples, int n_frames, const fsea_chain_stage *stage,
                          const fsea_chain_outputs *d_outputs, void *stream) {
    if (!c) return fail(FSEA_EINVAL, "chain is NULL");
    const fsea_chain_stage &st = stage ? *stage : NO_STAGE;
    const fsea_chain_outputs &o = d_outputs ? *d_outputs : NO_OUTPUTS;
    int rc = check_stage(st, n_samples, n_frames);
    if (!rc) rc = check_outputs(o, n_samples + st.n_zero, n_frames, true);
    if (rc) return rc;
    if (n_frames == 0) return FSEA_OK;
    if (n_samples && !d_iq) return fail(FSEA_EINVAL, "NULL buffer");
    rc = fsea_detail::check_aligned16("d_iq", d_iq);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t total = n_samples + st.n_zero;
    std::lock_guard<std::mutex> lock(c->mu);
    FSEA_ON_DEVICE(c->device);
    rc = reserve_pairs(c, total * 8 * (size_t)n_frames);
    if (rc) return rc;
    c->n_pairs = 0;   // from here on the buffer is being overwritten
    rc = queue_filter(c, 0, d_iq, n_samples, n_frames, st, s);
    if (rc) return rc;
    c->n_pairs = total;
    rc = queue_images(c, n_frames, o, o.points, o.lines, s);
    if (rc) return rc;
    if (o.pairs && total) {
        FSEA_HIP(hipMemcpyAsync(o.pairs, c->pairs.ptr, total * 8 * (size_t)n_frames, hipMemcpyDeviceToDevice, s));
    }
    return FSEA_OK;
}

}  // extern "C"
