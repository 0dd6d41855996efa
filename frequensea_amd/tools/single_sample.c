/*
 * fsea-single-sample -- the IQ trace movie: one capture drawn a few samples at a time, one image per step.
 *
 * Re-statement of c/single-sample.c:80-155 with its constants as defaults: frame n (from 1) fades the 1920 x 1080 canvas by
 * -f, joins the points of bytes [(n - 1) S, n S) of the capture with lines in the 1024 x 1024 IQ square at its centre, each
 * hit adding -p unless that reaches 255, and is written as OUT/sample-<n>.png through write_gray_png.  The frames are
 * fsea_trace_frames_host (include/fsea.h), CHUNK_FRAMES at a time.  With -v nothing is written but the canvas after the
 * last frame, as sample-<frames + 1>.png (the reference's name for it).
 * Deliberate differences:
 *   -p outside [1, 254], -f outside [0, 255] and -s < 1 are errors (the reference wraps pixels, fades upward or never ends);
 *   a missing capture is an error (the reference asserts);
 *   where the reference reads past its buffer (a size that is no multiple of -s, or an odd -s on the last frame), a frame is
 *   drawn only as far as both bytes of a point lie inside the file.
 *
 * usage: fsea-single-sample [-p N] [-s N] [-f N] [-v] [--out DIR] [--raw] [--frames N] [--width W] [--height H]
 *                           [--multiplier M] [--device D] capture.raw
 *   --raw      writes OUT/sample-<n>.raw (W H bytes) instead of PNG files
 *   --frames   stops after N frames
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

#define CHUNK_FRAMES 16 /* frames per fsea_trace_frames_host call */

static void usage_error(const char *msg) { tool_usage_error("fsea-single-sample", msg); }

static void die(const char *what) { tool_die("fsea-single-sample", what); }

static int write_frame(const char *out_dir, int raw, long index, int width, int height, const uint8_t *image) {
    char fname[1100];
    const size_t bytes = (size_t)width * height;
    if (raw) {
        snprintf(fname, sizeof(fname), "%s/sample-%ld.raw", out_dir, index);
        FILE *fp = fopen(fname, "wb");
        if (fp == NULL || fwrite(image, 1, bytes, fp) != bytes || fclose(fp) != 0) {
            fprintf(stderr, "fsea-single-sample: cannot write %s\n", fname);
            return 1;
        }
        return 0;
    }
    snprintf(fname, sizeof(fname), "%s/sample-%ld.png", out_dir, index);
    return write_gray_png(fname, width, height, image) != 0;
}

int main(int argc, char **argv) {
    const char *out_dir = "_export", *capture = NULL;
    long samples_step = 100, max_frames = -1;
    int raw = 0, preview = 0, device = 0;
    fsea_trace_config cfg = {1920, 1080, 4, 4, 0};
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--raw")) raw = 1;
        else if (!strcmp(argv[i], "-v")) preview = 1;
        else if (!strcmp(argv[i], "-p") && more) cfg.pixel_inc = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-s") && more) samples_step = atol(argv[++i]);
        else if (!strcmp(argv[i], "-f") && more) cfg.fade = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--out") && more) out_dir = argv[++i];
        else if (!strcmp(argv[i], "--frames") && more) max_frames = atol(argv[++i]);
        else if (!strcmp(argv[i], "--width") && more) cfg.width = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--height") && more) cfg.height = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--multiplier") && more) cfg.size_multiplier = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--device") && more) device = atoi(argv[++i]);
        else if (argv[i][0] != '-' && capture == NULL) capture = argv[i];
        else usage_error("usage: fsea-single-sample [-p pixel_inc] [-s samples_per_frame] [-f fade_per_frame] [-v (preview)] "
                         "[--out DIR] [--raw] [--frames N] [--width W] [--height H] [--multiplier M] [--device D] rfdata.raw");
    }
    if (capture == NULL) usage_error("no capture file given");
    if (cfg.pixel_inc < 1 || cfg.pixel_inc > 254) usage_error("-p must be in [1, 254]");
    if (cfg.fade < 0 || cfg.fade > 255) usage_error("-f must be in [0, 255]");
    if (samples_step < 1 || samples_step > 0x7fffffffL) usage_error("-s must be in [1, 2^31 - 1]");
    if (cfg.size_multiplier < 1 || cfg.size_multiplier > FSEA_IQ_MAX_MULTIPLIER) usage_error("--multiplier must be in [1, 16]");
    if (cfg.width < 256 * cfg.size_multiplier || cfg.height < 256 * cfg.size_multiplier || cfg.width > 16384 || cfg.height > 16384) {
        usage_error("--width and --height must hold the IQ square of 256 x multiplier pixels and be at most 16384");
    }

    FILE *fp = fopen(capture, "rb");
    if (fp == NULL) {
        fprintf(stderr, "fsea-single-sample: cannot open capture %s\n", capture);
        return EXIT_FAILURE;
    }
    fseek(fp, 0L, SEEK_END);
    const long size = ftell(fp);
    rewind(fp);
    uint8_t *samples = (uint8_t *)malloc(size > 0 ? (size_t)size : 1);
    if (samples == NULL) usage_error("out of memory");
    if (size < 0 || fread(samples, 1, (size_t)size, fp) != (size_t)size) {
        fprintf(stderr, "fsea-single-sample: cannot read capture %s\n", capture);
        return EXIT_FAILURE;
    }
    fclose(fp);
    printf("Size: %ld\n", size);

    const size_t step = (size_t)samples_step, frame_bytes = (size_t)cfg.width * cfg.height;
    long frames = (long)(((size_t)size + step - 1) / step); /* the reference's j = 0, S, 2 S, ... < size */
    if (max_frames >= 0 && frames > max_frames) frames = max_frames;
    uint8_t *images = (uint8_t *)malloc(frame_bytes * (preview ? 1 : CHUNK_FRAMES));
    if (images == NULL) usage_error("out of memory");
    fsea_trace *trace = NULL;
    if (fsea_trace_create(&trace, &cfg, device) != FSEA_OK) die("fsea_trace_create");

    for (long f0 = 0; f0 < frames; f0 += CHUNK_FRAMES) {
        const int n = (int)(frames - f0 < CHUNK_FRAMES ? frames - f0 : CHUNK_FRAMES);
        const size_t first = (size_t)f0 * step;
        if (fsea_trace_frames_host(trace, samples + first, (size_t)size - first, 1, step, n, preview ? NULL : images) != FSEA_OK) {
            die("fsea_trace_frames_host");
        }
        for (int k = 0; k < n && !preview; k++) {
            if (write_frame(out_dir, raw, f0 + k + 1, cfg.width, cfg.height, images + (size_t)k * frame_bytes)) return EXIT_FAILURE;
        }
    }
    if (preview) {
        if (fsea_trace_canvas_host(trace, images) != FSEA_OK) die("fsea_trace_canvas_host");
        if (write_frame(out_dir, raw, frames + 1, cfg.width, cfg.height, images)) return EXIT_FAILURE;
    }
    fsea_trace_destroy(trace);
    free(images);
    free(samples);
    return 0;
}
