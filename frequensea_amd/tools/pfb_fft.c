/*
 * fsea-pfb-fft -- a waterfall of a recording through a polyphase filter bank: M channels, a row every M / Q samples.
 *
 * The reference's spectrum tools transform rectangular frames (c/fft-batch.c: rate / N per bin, a sinc's side lobes in every
 * other bin).  This one reads a raw HackRF int8 recording whole and makes one fsea_pfb_run_host call (include/fsea.h) in
 * DB10_U8 mode with the prototype of fsea_pfb_prototype(M, P): column k of a row is the band centred at (k - M/2) rate / M
 * with the prototype's stop band.  The rows are written as an 8-bit grey PNG of width M through write_gray_png, row 0 the
 * first in time, and the row count, the channel width rate / M and the row rate rate / (M / Q) are printed.  With --channel K
 * --series FILE a second object in COMPLEX mode gives column K as a complex series (interleaved f32, one value per row).
 *
 * usage: fsea-pfb-fft FILE [--rate HZ] --channels M [--taps P] [--oversampling Q] [--out PNG] [--channel K --series FILE]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

static const char *USAGE =
    "usage: fsea-pfb-fft FILE [--rate HZ] --channels M [--taps P] [--oversampling Q] [--out PNG] [--channel K --series FILE]\n"
    "  FILE is a raw HackRF int8 IQ recording; it is split into M channels (M even) by a polyphase filter bank with P taps per\n"
    "  branch, a row every M / Q samples (Q 1, 2 or 4); the dB rows go to an 8-bit grey PNG of width M, first row first;\n"
    "  --channel K --series FILE also writes column K as interleaved f32 (re, im), one value per row\n"
    "  defaults: --rate 10000000 --taps 8 --oversampling 1 --out pfb.png";

static void usage_error(const char *msg) { tool_usage_error("fsea-pfb-fft", msg); }

static void die(const char *what) { tool_die("fsea-pfb-fft", what); }

int main(int argc, char **argv) {
    const char *out = "pfb.png", *path = NULL, *series_path = NULL;
    double rate = 10000000.0;
    int channels = 0, taps = 8, oversampling = 1, channel = -1;
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--help")) {
            puts(USAGE);
            return 0;
        } else if (!strcmp(argv[i], "--rate") && more) rate = atof(argv[++i]);
        else if (!strcmp(argv[i], "--channels") && more) channels = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--taps") && more) taps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--oversampling") && more) oversampling = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--out") && more) out = argv[++i];
        else if (!strcmp(argv[i], "--channel") && more) channel = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--series") && more) series_path = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    if (path == NULL) usage_error("no recording file given");
    if (!(rate > 0.0) || !isfinite(rate)) usage_error("--rate must be a positive number");
    if (channels < 2 || channels > FSEA_PFB_MAX_CHANNELS || channels % 2 != 0) usage_error("--channels must be even and in [2, 16384]");
    if (taps < 1 || taps > FSEA_PFB_MAX_BRANCH_TAPS) usage_error("--taps must be in [1, 16]");
    if ((oversampling != 1 && oversampling != 2 && oversampling != 4) || channels % oversampling != 0) {
        usage_error("--oversampling must be 1, 2 or 4 and divide --channels");
    }
    if ((channel >= 0) != (series_path != NULL)) usage_error("--channel and --series go together");
    if (channel >= channels) usage_error("--channel must be below --channels");

    FILE *fp = fopen(path, "rb");
    if (fp == NULL) {
        fprintf(stderr, "fsea-pfb-fft: cannot open recording %s\n", path);
        return EXIT_FAILURE;
    }
    fseek(fp, 0L, SEEK_END);
    const long size = ftell(fp);
    rewind(fp);
    const size_t n_samples = size > 0 ? (size_t)size / 2 : 0;
    uint8_t *iq = (uint8_t *)malloc(n_samples > 0 ? 2 * n_samples : 1);
    if (iq == NULL) usage_error("out of memory");
    if (fread(iq, 1, 2 * n_samples, fp) != 2 * n_samples) {
        fprintf(stderr, "fsea-pfb-fft: cannot read recording %s\n", path);
        return EXIT_FAILURE;
    }
    fclose(fp);

    double *c = (double *)malloc(sizeof(double) * (size_t)channels * (size_t)taps);
    if (c == NULL) usage_error("out of memory");
    if (fsea_pfb_prototype(channels, taps, c) != FSEA_OK) die("fsea_pfb_prototype");
    fsea_pfb *pfb = NULL;
    if (fsea_pfb_create(&pfb, c, channels, taps, oversampling, FSEA_MODE_DB10_U8, 0) != FSEA_OK) die("fsea_pfb_create");
    const size_t rows = fsea_pfb_out_frames(pfb, n_samples);
    if (rows < 1) {
        fprintf(stderr, "fsea-pfb-fft: recording %s holds %zu samples, fewer than one row of %d\n", path, n_samples,
                channels / oversampling);
        return EXIT_FAILURE;
    }
    if (rows > 0x7fffffffu / (size_t)channels) usage_error("the image would hold more than 2^31 pixels");
    uint8_t *image = (uint8_t *)malloc(rows * fsea_pfb_row_bytes(pfb));
    if (image == NULL) usage_error("out of memory");
    if (fsea_pfb_run_host(pfb, iq, n_samples, 1, image, NULL, NULL) != FSEA_OK) die("fsea_pfb_run_host");
    fsea_pfb_destroy(pfb);
    printf("rows %zu\nchannel width %.6f Hz\nrow rate %.6f Hz\n", rows, rate / (double)channels,
           rate / (double)(channels / oversampling));
    if (write_gray_png(out, channels, (int)rows, image) != 0) {
        fprintf(stderr, "fsea-pfb-fft: cannot write %s\n", out);
        return EXIT_FAILURE;
    }
    free(image);

    if (series_path != NULL) {
        /* the same stream through a second object in COMPLEX mode: its transposed rows hold channel K in a row */
        if (fsea_pfb_create(&pfb, c, channels, taps, oversampling, FSEA_MODE_COMPLEX_F32, 0) != FSEA_OK) die("fsea_pfb_create");
        float *spectra = (float *)malloc(rows * fsea_pfb_row_bytes(pfb));
        float *series = (float *)malloc(rows * fsea_pfb_row_bytes(pfb));
        if (spectra == NULL || series == NULL) usage_error("out of memory");
        if (fsea_pfb_run_host(pfb, iq, n_samples, 1, spectra, NULL, series) != FSEA_OK) die("fsea_pfb_run_host");
        fsea_pfb_destroy(pfb);
        FILE *sp = fopen(series_path, "wb");
        if (sp == NULL || fwrite(series + 2 * (size_t)channel * rows, sizeof(float), 2 * rows, sp) != 2 * rows || fclose(sp) != 0) {
            fprintf(stderr, "fsea-pfb-fft: cannot write %s\n", series_path);
            return EXIT_FAILURE;
        }
        free(spectra);
        free(series);
    }
    free(c);
    free(iq);
    return 0;
}
