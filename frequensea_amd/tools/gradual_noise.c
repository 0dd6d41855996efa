/*
 * fsea-gradual-noise -- the gradual noise movie: eased cross-fades between consecutive capture files, one image per step.
 *
 * Re-statement of c/gradual-noise.c:85-123 with its constants as defaults:
 *   pair k blends the I bytes of the captures at START + k FSTEP and START + (k + 1) FSTEP MHz (the frequency is the
 *   reference's running sum), one frame per t = 0, STEP, 2 STEP, ... while the running sum stays below 1.0 (100 frames for
 *   0.01); the frame's weight is sine_ease_in_out(t) = 0.5 (1 - cos(t pi)), computed here with libm; the frame itself is
 *   fsea_interp_image_frames_host (include/fsea.h): every sample blown up by BLOCK_SCALE = max(W, H) / IQ.
 *   Frames are written as OUT/noise-<n>.png, n from 1, through write_gray_png.
 * Only the first 2 IQ^2 bytes of a capture are read (the reference reads 2 W H bytes and uses those).  A missing or short
 * capture is an error (the reference crashes on the NULL FILE *), and the pair after the last frame is not read.
 *
 * usage: fsea-gradual-noise [--dir DIR] [--pattern rf-%.3f-big.raw] [--start MHZ] [--freq-step MHZ] [--step S]
 *                           [--frames N] [--width W] [--height H] [--iq-size IQ] [--out DIR] [--raw] [--device D]
 *                           [--print-weights]
 *   --raw            writes OUT/noise-<n>.raw (W H bytes) instead of PNG files
 *   --print-weights  prints the eased weights of one pair, one "%a" per line, and exits (needs no GPU)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

#define PI 3.14159265358979323846 /* glibc's M_PI */
#define CHUNK_FRAMES 16           /* frames per fsea_interp_image_frames_host call */
#define MAX_PAIR_FRAMES (1 << 20)

static void usage_error(const char *msg) { tool_usage_error("fsea-gradual-noise", msg); }

static void die(const char *what) { tool_die("fsea-gradual-noise", what); }

static double sine_ease_in_out(double p) { return 0.5 * (1 - cos(p * PI)); }

/* the eased weights of one pair: t from 0 in steps of `step` until the running sum reaches 1.0 */
static int pair_weights(double step, double **weights) {
    int n = 0;
    double t = 0.0;
    do {
        ++n;
        t += step;
    } while (!(t >= 1.0) && n < MAX_PAIR_FRAMES);
    if (!(t >= 1.0)) usage_error("--step gives more than 2^20 frames per pair");
    double *w = (double *)malloc(sizeof(double) * (size_t)n);
    if (w == NULL) usage_error("out of memory");
    t = 0.0;
    for (int i = 0; i < n; i++) {
        w[i] = sine_ease_in_out(t);
        t += step;
    }
    *weights = w;
    return n;
}

/* one "%...f" conversion and nothing else that printf would interpret */
static int pattern_ok(const char *p) {
    const char *c = strchr(p, '%');
    if (c == NULL || strchr(c + 1, '%') != NULL) return 0;
    ++c;
    while ((*c >= '0' && *c <= '9') || *c == '.') ++c;
    return *c == 'f';
}

static void read_capture(uint8_t *dst, size_t bytes, const char *dir, const char *pattern, double freq_mhz) {
    char name[256], path[1024];
    snprintf(name, sizeof(name), pattern, freq_mhz);
    snprintf(path, sizeof(path), "%s/%s", dir, name);
    FILE *fp = fopen(path, "rb");
    if (fp == NULL) {
        fprintf(stderr, "fsea-gradual-noise: cannot open capture %s\n", path);
        exit(EXIT_FAILURE);
    }
    const size_t got = fread(dst, 1, bytes, fp);
    fclose(fp);
    if (got != bytes) {
        fprintf(stderr, "fsea-gradual-noise: capture %s holds %zu bytes, %zu are needed\n", path, got, bytes);
        exit(EXIT_FAILURE);
    }
}

int main(int argc, char **argv) {
    const char *dir = "../rftmp", *pattern = "rf-%.3f-big.raw", *out_dir = "_export";
    double freq_mhz = 1.0, freq_step = 0.01, step = 0.01;
    int total_frames = 20000, raw = 0, device = 0, print_weights = 0;
    fsea_interp_geometry geo = {1920, 1080, 256, 1}; /* the tool's (b + 128) % 256 is flip */
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--raw")) raw = 1;
        else if (!strcmp(argv[i], "--print-weights")) print_weights = 1;
        else if (!strcmp(argv[i], "--dir") && more) dir = argv[++i];
        else if (!strcmp(argv[i], "--pattern") && more) pattern = argv[++i];
        else if (!strcmp(argv[i], "--out") && more) out_dir = argv[++i];
        else if (!strcmp(argv[i], "--start") && more) freq_mhz = atof(argv[++i]);
        else if (!strcmp(argv[i], "--freq-step") && more) freq_step = atof(argv[++i]);
        else if (!strcmp(argv[i], "--step") && more) step = atof(argv[++i]);
        else if (!strcmp(argv[i], "--frames") && more) total_frames = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--width") && more) geo.width = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--height") && more) geo.height = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--iq-size") && more) geo.iq_size = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--device") && more) device = atoi(argv[++i]);
        else usage_error("usage: fsea-gradual-noise [--dir DIR] [--pattern PAT] [--start MHZ] [--freq-step MHZ] [--step S] "
                         "[--frames N] [--width W] [--height H] [--iq-size IQ] [--out DIR] [--raw] [--device D] [--print-weights]");
    }
    if (!(step > 0.0)) usage_error("--step must be > 0");
    if (total_frames < 0) usage_error("--frames must be >= 0");
    if (!pattern_ok(pattern)) usage_error("--pattern must hold one %f conversion, as rf-%.3f-big.raw");

    double *weights = NULL;
    const int pair_frames = pair_weights(step, &weights);
    if (print_weights) {
        for (int i = 0; i < pair_frames; i++) printf("%a\n", weights[i]);
        return 0;
    }

    /* the tables check the geometry before any allocation depends on it */
    int32_t *tab = (int32_t *)malloc(sizeof(int32_t) * 2 * 16384);
    if (tab == NULL) usage_error("out of memory");
    if (fsea_interp_image_tables(geo.width, geo.height, geo.iq_size, tab, tab + 16384) != FSEA_OK) die("geometry");
    free(tab);

    const size_t block_bytes = 2 * (size_t)geo.iq_size * geo.iq_size, frame_bytes = (size_t)geo.width * geo.height;
    uint8_t *block = (uint8_t *)malloc(block_bytes);
    uint8_t *images = (uint8_t *)malloc(frame_bytes * CHUNK_FRAMES);
    if (block == NULL || images == NULL) usage_error("out of memory");
    fsea_interp *interp = NULL;
    if (fsea_interp_create(&interp, FSEA_IQ_U8, block_bytes, device) != FSEA_OK) die("fsea_interp_create");

    int frame = 1;
    for (int pair = 0; frame <= total_frames; pair++) {
        if (pair == 0) {
            read_capture(block, block_bytes, dir, pattern, freq_mhz);
            if (fsea_interp_push_host(interp, block) != FSEA_OK) die("fsea_interp_push_host");
        } else {
            freq_mhz += freq_step;
            printf("Frequency: %.3f\n", freq_mhz);
        }
        /* the second capture of a pair is the first of the next: A takes what B held */
        read_capture(block, block_bytes, dir, pattern, freq_mhz + freq_step);
        if (fsea_interp_push_host(interp, block) != FSEA_OK) die("fsea_interp_push_host");
        for (int f0 = 0; f0 < pair_frames && frame <= total_frames; f0 += CHUNK_FRAMES) {
            int n = pair_frames - f0 < CHUNK_FRAMES ? pair_frames - f0 : CHUNK_FRAMES;
            if (n > total_frames - frame + 1) n = total_frames - frame + 1;
            if (fsea_interp_image_frames_host(interp, weights + f0, n, &geo, images) != FSEA_OK) die("fsea_interp_image_frames_host");
            for (int k = 0; k < n; k++, frame++) {
                char fname[1100];
                if (raw) {
                    snprintf(fname, sizeof(fname), "%s/noise-%d.raw", out_dir, frame);
                    FILE *fp = fopen(fname, "wb");
                    if (fp == NULL || fwrite(images + (size_t)k * frame_bytes, 1, frame_bytes, fp) != frame_bytes || fclose(fp) != 0) {
                        fprintf(stderr, "fsea-gradual-noise: cannot write %s\n", fname);
                        return EXIT_FAILURE;
                    }
                } else {
                    snprintf(fname, sizeof(fname), "%s/noise-%d.png", out_dir, frame);
                    if (write_gray_png(fname, geo.width, geo.height, images + (size_t)k * frame_bytes) != 0) return EXIT_FAILURE;
                }
            }
        }
    }
    fsea_interp_destroy(interp);
    free(images);
    free(block);
    free(weights);
    return 0;
}
