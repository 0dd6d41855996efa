// fsea_capture.hip -- the reference's signal scene on a resident recording (include/fsea.h: fsea_capture_*;
// lua/signal-detector.lua:89-133): detect the bursts, low-pass the blocks of each burst, keep them appended on the device,
// draw a burst as a line image.
//
// No kernel lives here.  A scan queues the detector launch (fsea_detect_u8_device) and the copy of its 24 bytes per block,
// waits, runs the scene's state machine over the statistics on the host (fsea_capture_segment) and then queues one
// fsea_chain_run_device per run of consecutive gated blocks, straight from the recording, its pairs going to the end of the
// burst buffer.  The block sequence it replaces brings every block to the host to decide whether it is worth filtering.
#include "fsea_fir_stage.h"

#include <algorithm>
#include <cstring>
#include <vector>

using fsea_detail::DeviceGuard;
using fsea_detail::fail;

struct fsea_capture {
    int device = 0;
    mutable std::mutex mu;                  // the accessors lock it too
    fsea_detail::HostStaging staging;       // the host forms' stream and the images' way back
    fsea_detail::DeviceBuffer recording;    // scan_host's upload
    fsea_detail::DeviceBuffer d_sums;
    fsea_detail::PinnedBuffer h_sums;
    std::vector<double> mean, sd;           // of the last scan's blocks
    struct Burst {
        size_t first_block, n_blocks, n_pairs, at;   // `at`: its first pair in the burst buffer
        bool open;
    };
    std::vector<Burst> bursts;
    fsea_detail::DeviceBuffer pairs;        // the bursts' pairs, one after the other
    size_t pairs_used = 0;                  // in pairs
    size_t blocks_seen = 0;                 // of all scans since reset
    // the inner objects are the first to go: the detector, the chain, the drawer
    fsea_detail::Owned<fsea_iq_draw, fsea_iq_draw_destroy> draw;
    fsea_detail::Owned<fsea_chain, fsea_chain_destroy> chain;
    fsea_detail::Owned<fsea_detect, fsea_detect_destroy> detect;

    float *d_pairs() const { return static_cast<float *>(pairs.ptr); }
};

namespace {

constexpr size_t RUN_SAMPLES = (size_t)1 << 25;   // samples per filter launch at most: bounds the chain's own buffer

int check_scan(const fsea_capture *c, const void *iq, size_t block_bytes, size_t n_blocks) {
    if (!c) return fail(FSEA_EINVAL, "capture is NULL");
    if (block_bytes < 16 || (block_bytes & 15) || block_bytes > ((size_t)1 << 31)) {
        return fail(FSEA_EINVAL, "block_bytes must be a multiple of 16 in [16, 2^31], got %zu", block_bytes);
    }
    if (n_blocks == 0 || n_blocks > ((size_t)1 << 40) / block_bytes) {
        return fail(FSEA_EINVAL, "n_blocks must be at least 1 and the blocks at most 2^40 bytes, got %zu x %zu", n_blocks,
                    block_bytes);
    }
    if (!iq) return fail(FSEA_EINVAL, "NULL buffer");
    return FSEA_OK;
}

// room for `more` pairs behind the ones in use, which move along; the device is idle (every scan ends with a wait)
int reserve_pairs(fsea_capture *c, size_t more) { return c->pairs.grow((c->pairs_used + more) * 8, c->pairs_used * 8); }

// The caller holds c->mu and is on c's device.
int scan(fsea_capture *c, const uint8_t *d_iq, size_t block_bytes, size_t n_blocks, int flip, double threshold, hipStream_t s) {
    int rc = c->d_sums.grow(24 * n_blocks);
    if (!rc) rc = c->h_sums.grow(24 * n_blocks);
    if (rc) return rc;
    uint64_t *d_sums = static_cast<uint64_t *>(c->d_sums.ptr), *h_sums = static_cast<uint64_t *>(c->h_sums.ptr);
    rc = fsea_detect_u8_device(c->detect, d_iq, block_bytes, n_blocks, flip, d_sums, s);
    if (rc) return rc;
    FSEA_HIP(hipMemcpyAsync(h_sums, d_sums, 24 * n_blocks, hipMemcpyDeviceToHost, s));
    FSEA_HIP(hipStreamSynchronize(s));

    c->mean.assign(n_blocks, 0.0);
    c->sd.assign(n_blocks, 0.0);
    for (size_t b = 0; b < n_blocks; ++b) {
        rc = fsea_detect_finish(h_sums + 3 * b, block_bytes, &c->mean[b], &c->sd[b]);
        if (rc) return rc;
    }
    std::vector<fsea_capture_run> runs(n_blocks / 2 + 1);
    size_t n_runs = 0;
    const bool was_open = !c->bursts.empty() && c->bursts.back().open;
    rc = fsea_capture_segment(c->sd.data(), n_blocks, threshold, was_open, runs.data(), &n_runs);
    if (rc) return rc;

    const size_t n_samples = block_bytes / 2;
    size_t gated = 0;
    for (size_t r = 0; r < n_runs; ++r) gated += runs[r].n_blocks;
    if (gated > (((size_t)1 << 40) - c->pairs_used) / n_samples) return fail(FSEA_EINVAL, "the bursts exceed 2^40 pairs");
    rc = reserve_pairs(c, gated * n_samples);
    if (rc) return rc;

    fsea_chain_stage stage;
    std::memset(&stage, 0, sizeof(stage));
    stage.flip = flip;
    const size_t per_launch = std::max<size_t>(1, std::min<size_t>(RUN_SAMPLES / n_samples, 0x7fffffff));
    for (size_t r = 0; r < n_runs; ++r) {
        const fsea_capture_run &run = runs[r];
        if (!run.continues) c->bursts.push_back({c->blocks_seen + run.first_block, 0, 0, c->pairs_used, true});
        fsea_capture::Burst &burst = c->bursts.back();
        for (size_t f0 = 0; f0 < run.n_blocks; f0 += per_launch) {
            const size_t nf = std::min(per_launch, run.n_blocks - f0);
            // The chain filters into its own buffer and copies from there (one more write and read of the pairs).  Where a
            // longer run makes it reallocate that buffer, the hipFree inside waits for the copy still queued on s.
            fsea_chain_outputs out;
            std::memset(&out, 0, sizeof(out));
            out.size_multiplier = 1;
            out.pairs = c->d_pairs() + 2 * c->pairs_used;
            rc = fsea_chain_run_device(c->chain, d_iq + (run.first_block + f0) * block_bytes, n_samples, (int)nf, &stage, &out, s);
            if (rc) return rc;
            c->pairs_used += nf * n_samples;
            burst.n_pairs += nf * n_samples;
            burst.n_blocks += nf;
        }
        burst.open = run.open != 0;
    }
    c->blocks_seen += n_blocks;
    FSEA_HIP(hipStreamSynchronize(s));
    return FSEA_OK;
}

int check_burst(const fsea_capture *c, size_t burst) {
    if (burst >= c->bursts.size()) return fail(FSEA_EINVAL, "burst %zu out of range [0, %zu)", burst, c->bursts.size());
    return FSEA_OK;
}

int check_lines(const fsea_capture *c, int size_multiplier) {
    if (!c) return fail(FSEA_EINVAL, "capture is NULL");
    return fsea_detail::check_multiplier(size_multiplier);
}

// the caller holds c->mu
int lines_launch(fsea_capture *c, size_t burst, int m, size_t n_line_points, void *d_image, hipStream_t s) {
    int rc = check_burst(c, burst);
    if (rc) return rc;
    const fsea_capture::Burst &b = c->bursts[burst];
    if (n_line_points > b.n_pairs) {
        return fail(FSEA_EINVAL, "n_line_points %zu exceeds the %zu pairs of the burst", n_line_points, b.n_pairs);
    }
    return fsea_iq_lines_device(c->draw, c->d_pairs() + 2 * b.at, FSEA_IQ_F32, 0, n_line_points, 1, m, d_image, s);
}

}  // namespace

extern "C" {

int fsea_capture_create(fsea_capture **out, const double *taps, int n_taps, int device) {
    if (!out) return fail(FSEA_EINVAL, "capture out-pointer is NULL");
    *out = nullptr;
    if (int rc = fsea_stage::FirState::check_taps(taps, n_taps)) return rc;   // bad taps are reported before a missing device
    return fsea_detail::create_object(out, device, "fsea_capture_create", [&](fsea_capture *c) -> int {
        int rc = fsea_chain_create(&c->chain.ptr, taps, n_taps, device);
        if (!rc) rc = fsea_detect_create(&c->detect.ptr, device);
        return rc ? rc : fsea_iq_draw_create(&c->draw.ptr, device);
    });
}

int fsea_capture_destroy(fsea_capture *c) { return fsea_detail::destroy_object(c); }

int fsea_capture_reset(fsea_capture *c) {
    if (!c) return fail(FSEA_EINVAL, "capture is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    c->bursts.clear();
    c->mean.clear();
    c->sd.clear();
    c->pairs_used = c->blocks_seen = 0;
    return fsea_chain_reset(c->chain);   // waits for the device
}

int fsea_capture_scan_device(fsea_capture *c, const void *d_iq, size_t block_bytes, size_t n_blocks, int flip,
                             double threshold, void *stream) {
    int rc = check_scan(c, d_iq, block_bytes, n_blocks);
    if (!rc) rc = fsea_detail::check_aligned16("d_iq", d_iq);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    FSEA_ON_DEVICE(c->device);
    return scan(c, static_cast<const uint8_t *>(d_iq), block_bytes, n_blocks, flip, threshold, static_cast<hipStream_t>(stream));
}

int fsea_capture_scan_host(fsea_capture *c, const uint8_t *iq, size_t block_bytes, size_t n_blocks, int flip,
                           double threshold) {
    int rc = check_scan(c, iq, block_bytes, n_blocks);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    FSEA_ON_DEVICE(c->device);
    rc = c->recording.grow(block_bytes * n_blocks);
    if (rc) return rc;
    hipStream_t s = c->staging.stream;
    FSEA_HIP(hipMemcpyAsync(c->recording.ptr, iq, block_bytes * n_blocks, hipMemcpyHostToDevice, s));
    return scan(c, static_cast<const uint8_t *>(c->recording.ptr), block_bytes, n_blocks, flip, threshold, s);
}

int fsea_capture_segment(const double *sd, size_t n_blocks, double threshold, int capturing, fsea_capture_run *runs,
                         size_t *n_runs) {
    if (!n_runs) return fail(FSEA_EINVAL, "NULL buffer");
    *n_runs = 0;
    if ((n_blocks && !sd) || !runs) return fail(FSEA_EINVAL, "NULL buffer");
    size_t n = 0;
    if (capturing) runs[n++] = fsea_capture_run{0, 0, 1, 1};
    bool in_run = capturing != 0;
    for (size_t b = 0; b < n_blocks; ++b) {
        if (sd[b] > threshold) {   // false for a NaN
            if (!in_run) runs[n++] = fsea_capture_run{b, 0, 0, 1};
            in_run = true;
            runs[n - 1].n_blocks++;
        } else if (in_run) {       // this block ends the burst and is dropped
            runs[n - 1].open = 0;
            in_run = false;
        }
    }
    *n_runs = n;
    return FSEA_OK;
}

size_t fsea_capture_n_blocks(const fsea_capture *c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    return c->sd.size();
}

int fsea_capture_stats(const fsea_capture *c, size_t block, double *mean, double *sd) {
    if (!c) return fail(FSEA_EINVAL, "capture is NULL");
    if (!mean || !sd) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(c->mu);
    if (block >= c->sd.size()) return fail(FSEA_EINVAL, "block %zu out of range [0, %zu)", block, c->sd.size());
    *mean = c->mean[block];
    *sd = c->sd[block];
    return FSEA_OK;
}

size_t fsea_capture_n_bursts(const fsea_capture *c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    return c->bursts.size();
}

int fsea_capture_burst(const fsea_capture *c, size_t burst, fsea_capture_burst_info *info) {
    if (!c) return fail(FSEA_EINVAL, "capture is NULL");
    if (!info) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(c->mu);
    int rc = check_burst(c, burst);
    if (rc) return rc;
    const fsea_capture::Burst &b = c->bursts[burst];
    *info = fsea_capture_burst_info{b.first_block, b.n_blocks, b.n_pairs, b.open ? 1 : 0, c->d_pairs() + 2 * b.at};
    return FSEA_OK;
}

int fsea_capture_burst_pairs_host(fsea_capture *c, size_t burst, float *pairs) {
    if (!c) return fail(FSEA_EINVAL, "capture is NULL");
    if (!pairs) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(c->mu);
    int rc = check_burst(c, burst);
    if (rc) return rc;
    const fsea_capture::Burst &b = c->bursts[burst];
    if (!b.n_pairs) return FSEA_OK;
    FSEA_ON_DEVICE(c->device);
    FSEA_HIP(hipMemcpyAsync(pairs, c->d_pairs() + 2 * b.at, b.n_pairs * 8, hipMemcpyDeviceToHost, c->staging.stream));
    FSEA_HIP(hipStreamSynchronize(c->staging.stream));
    return FSEA_OK;
}

int fsea_capture_burst_lines_device(fsea_capture *c, size_t burst, int size_multiplier, size_t n_line_points, void *d_image,
                                    void *stream) {
    int rc = check_lines(c, size_multiplier);
    if (rc) return rc;
    if (!d_image) return fail(FSEA_EINVAL, "NULL buffer");
    rc = fsea_detail::check_aligned16("d_image", d_image);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    return lines_launch(c, burst, size_multiplier, n_line_points, d_image, static_cast<hipStream_t>(stream));
}

int fsea_capture_burst_lines_host(fsea_capture *c, size_t burst, int size_multiplier, size_t n_line_points, uint8_t *image) {
    int rc = check_lines(c, size_multiplier);
    if (rc) return rc;
    if (!image) return fail(FSEA_EINVAL, "NULL buffer");
    std::lock_guard<std::mutex> lock(c->mu);
    rc = check_burst(c, burst);
    if (rc) return rc;
    FSEA_ON_DEVICE(c->device);
    const size_t pixels = (size_t)65536 * size_multiplier * size_multiplier;
    return c->staging.run(
        0, pixels, image, [](void *) {},
        [&](void *, void *d_out, hipStream_t s) { return lines_launch(c, burst, size_multiplier, n_line_points, d_out, s); });
}

}  // extern "C"
