/*
 * fsea-signal-capture -- the signal scene over a recording: find the bursts, low-pass them, draw each as a growing IQ line
 * image.
 *
 * Re-statement of lua/signal-detector.lua:89-133 with its constants as defaults, on the nrf_signal_capture block
 * (include/nrf.h): the recording is read whole and scanned once in blocks of --block-bytes; a block whose standard deviation
 * (nrf_signal_detector_process's) is above --threshold starts or continues a burst, the first one at or below it ends the
 * burst and is dropped; the blocks of a burst go through the low-pass filter (--sample-rate, --cutoff, --taps), one filter
 * for the whole recording.  One line per block is printed: index, mean, standard deviation and idle, start, captured or
 * end.  Burst b is then drawn as the scene draws it: frame k is nrf_buffer_to_iq_lines(burst, --multiplier, p) for
 * p = 0, STEP, 2 STEP, ... (a double accumulated by + STEP, passed as float) while p < 1, written as
 * OUT/burst-<b>-<k>.png (8-bit gray, the bytes of the line image) through write_gray_png on a writer thread.
 * The scene's shader gain (x 100) and its alpha fade are rendering and out of scope: the images hold the counts.
 * Deliberate differences: --flip takes raw HackRF int8 bytes (b ^ 0x80 first); a burst still open at the end of the
 * recording is drawn too (the scene would go on capturing).
 *
 * usage: fsea-signal-capture [--block-bytes N] [--threshold T] [--sample-rate HZ] [--cutoff HZ] [--taps N] [--multiplier M]
 *                            [--step S] [--flip] [--out-dir DIR] recording.raw
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "nrf.h"
#include "pipeline.h"
#include "tool_common.h"

#define MIN_STEP 0.0002 /* at most 5001 frames per burst: the file name has four digits */

static const char *USAGE =
    "usage: fsea-signal-capture [--block-bytes N] [--threshold T] [--sample-rate HZ] [--cutoff HZ] [--taps N] "
    "[--multiplier M] [--step S] [--flip] [--out-dir DIR] recording.raw\n"
    "  one line per block (index mean sd idle|start|captured|end), then OUT/burst-<b>-<k>.png per burst and frame:\n"
    "  the IQ line image of the burst's first p of its points, p = 0, S, 2 S, ... < 1\n"
    "  defaults: --block-bytes 262144 --threshold 100 --sample-rate 5000000 --cutoff 200000 --taps 97 --multiplier 4\n"
    "            --step 0.005 --out-dir _export\n"
    "  the scene's shader gain (x 100) and alpha fade are rendering and out of scope: the images hold the counts";

static void usage_error(const char *msg) { tool_usage_error("fsea-signal-capture", msg); }

int main(int argc, char **argv) {
    const char *out_dir = "_export", *path = NULL;
    long block_bytes = TRANSFER_BYTES;
    double threshold = 100.0, step = 0.005;
    int sample_rate = 5000000, cutoff = 200000, taps = 97, multiplier = 4, flip = 0;
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--help")) {
            puts(USAGE);
            return 0;
        } else if (!strcmp(argv[i], "--flip")) flip = 1;
        else if (!strcmp(argv[i], "--block-bytes") && more) block_bytes = atol(argv[++i]);
        else if (!strcmp(argv[i], "--threshold") && more) threshold = atof(argv[++i]);
        else if (!strcmp(argv[i], "--sample-rate") && more) sample_rate = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--cutoff") && more) cutoff = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--taps") && more) taps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--multiplier") && more) multiplier = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--step") && more) step = atof(argv[++i]);
        else if (!strcmp(argv[i], "--out-dir") && more) out_dir = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    if (path == NULL) usage_error("no recording file given");
    if (strlen(out_dir) > 500) usage_error("--out-dir is longer than 500 characters");
    if (block_bytes < 16 || block_bytes % 16 != 0 || block_bytes > 0x40000000L) {
        usage_error("--block-bytes must be a multiple of 16 in [16, 2^30]");
    }
    if (isnan(threshold)) usage_error("--threshold must be a number");
    if (sample_rate < 1) usage_error("--sample-rate must be >= 1");
    if (taps < 1 || taps > FSEA_FIR_MAX_TAPS) usage_error("--taps must be in [1, 512]");
    if (multiplier < 1 || multiplier > FSEA_IQ_MAX_MULTIPLIER) usage_error("--multiplier must be in [1, 16]");
    if (cutoff < 0 || cutoff > sample_rate / 2) usage_error("--cutoff must be in [0, sample-rate / 2]");
    if (!(step >= MIN_STEP) || !isfinite(step)) usage_error("--step must be a number of at least 0.0002");

    FILE *fp = fopen(path, "rb");
    if (fp == NULL) {
        fprintf(stderr, "fsea-signal-capture: cannot open recording %s\n", path);
        return EXIT_FAILURE;
    }
    fseek(fp, 0L, SEEK_END);
    const long size = ftell(fp);
    rewind(fp);
    const long n_blocks = size > 0 ? size / block_bytes : 0;
    if (n_blocks < 1) {
        fprintf(stderr, "fsea-signal-capture: recording %s holds %ld bytes, less than one block of %ld\n", path, size, block_bytes);
        return EXIT_FAILURE;
    }
    if (n_blocks * (block_bytes / 2) > 0x3fffffffL) usage_error("the recording holds more than 2^30 IQ pairs");
    const long used = n_blocks * block_bytes; /* a trailing partial block is ignored */
    nut_buffer *recording = nut_buffer_new_u8((int)(used / 2), 2, NULL);
    if (recording == NULL) usage_error("out of memory");
    if (fread(recording->data.u8, 1, (size_t)used, fp) != (size_t)used) {
        fprintf(stderr, "fsea-signal-capture: cannot read recording %s\n", path);
        return EXIT_FAILURE;
    }
    fclose(fp);
    if (flip) {
        for (long i = 0; i < used; i++) recording->data.u8[i] ^= 0x80;
    }

    nrf_signal_capture *capture = nrf_signal_capture_new(sample_rate, cutoff, taps, threshold);
    const int n_bursts = nrf_signal_capture_scan(capture, recording, (int)(block_bytes / 2));
    nut_buffer_free(recording);

    int capturing = 0;
    for (long b = 0; b < n_blocks; b++) {
        const double mean = nrf_signal_capture_get_mean(capture, (int)b);
        const double sd = nrf_signal_capture_get_standard_deviation(capture, (int)b);
        const int above = sd > threshold;
        printf("%ld %.17g %.17g %s\n", b, mean, sd, above ? (capturing ? "captured" : "start") : (capturing ? "end" : "idle"));
        capturing = above;
    }
    fflush(stdout);

    const int side = 256 * multiplier;
    const size_t pixels = (size_t)side * side;
    uint8_t *p0 = (uint8_t *)malloc(pixels), *p1 = (uint8_t *)malloc(pixels);
    png_writer writer;
    if (p0 == NULL || p1 == NULL || png_writer_start(&writer, p0, p1) != 0) usage_error("out of memory");
    for (int burst = 0; burst < n_bursts; burst++) {
        int k = 0;
        for (double p = 0.0; p < 1.0; p += step, k++) {
            nut_buffer *image = nrf_signal_capture_get_iq_lines(capture, burst, multiplier, (float)p);
            memcpy(png_writer_acquire(&writer), image->data.u8, pixels);
            nut_buffer_free(image);
            char name[600];
            snprintf(name, sizeof(name), "%s/burst-%03d-%04d.png", out_dir, burst, k);
            png_writer_submit(&writer, name, side, side);
        }
    }
    const int failed = png_writer_finish(&writer);
    nrf_signal_capture_free(capture);
    free(p0);
    free(p1);
    if (failed) {
        fprintf(stderr, "fsea-signal-capture: cannot write the images to %s\n", out_dir);
        return EXIT_FAILURE;
    }
    return 0;
}
