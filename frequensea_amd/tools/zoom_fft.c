/*
 * fsea-zoom-fft -- a zoomed waterfall of a recording: shift, low-pass, keep every D-th sample, transform.
 *
 * The reference's spectrum tools see the device's whole bandwidth (c/fft-batch.c: one row per transfer, rate / N per bin).
 * This one reads a raw HackRF int8 recording whole and makes one fsea_zoom_run_host call (include/fsea.h) in DB10_U8 mode:
 * the spectrum is moved up by --offset (a signal at +f is centred by --offset -f, nrf_freq_shifter_new's convention),
 * filtered by the low-pass of nrf_fir_get_low_pass_coefficients(--rate, --cutoff, --taps) and decimated by --decimation;
 * row r is the N-point spectrum of the decimated samples [r H, r H + N).  The rows are written as an 8-bit grey PNG of
 * width N through write_gray_png, row 0 the first in time, and the row count and the bin width rate / (D N) are printed.
 *
 * usage: fsea-zoom-fft FILE --rate HZ --offset HZ --decimation D --cutoff HZ --taps L --fft N [--hop H] [--out PNG]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

static const char *USAGE =
    "usage: fsea-zoom-fft FILE --rate HZ --offset HZ --decimation D --cutoff HZ --taps L --fft N [--hop H] [--out PNG]\n"
    "  FILE is a raw HackRF int8 IQ recording; the spectrum is moved up by --offset, low-passed at --cutoff with L taps,\n"
    "  decimated by D and transformed N points at a time every H decimated samples (default N); the dB rows go to an 8-bit\n"
    "  grey PNG of width N, first row first\n"
    "  defaults: --rate 10000000 --offset 0 --decimation 16 --cutoff rate / (2 D) --taps 97 --fft 128 --out zoom.png";

static void usage_error(const char *msg) { tool_usage_error("fsea-zoom-fft", msg); }

static void die(const char *what) { tool_die("fsea-zoom-fft", what); }

int main(int argc, char **argv) {
    const char *out = "zoom.png", *path = NULL;
    double rate = 10000000.0, offset = 0.0, cutoff = -1.0;
    int decimation = 16, taps = 97, fft_size = 128, hop = 0;
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--help")) {
            puts(USAGE);
            return 0;
        } else if (!strcmp(argv[i], "--rate") && more) rate = atof(argv[++i]);
        else if (!strcmp(argv[i], "--offset") && more) offset = atof(argv[++i]);
        else if (!strcmp(argv[i], "--decimation") && more) decimation = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--cutoff") && more) cutoff = atof(argv[++i]);
        else if (!strcmp(argv[i], "--taps") && more) taps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--fft") && more) fft_size = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--hop") && more) hop = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--out") && more) out = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    if (path == NULL) usage_error("no recording file given");
    if (!(rate > 0.0) || !isfinite(rate)) usage_error("--rate must be a positive number");
    if (!isfinite(offset)) usage_error("--offset must be a number");
    if (decimation < 1 || decimation > FSEA_ZOOM_MAX_DECIMATION) usage_error("--decimation must be in [1, 64]");
    if (taps < 1 || taps > FSEA_FIR_MAX_TAPS) usage_error("--taps must be in [1, 512]");
    if (cutoff < 0.0) cutoff = rate / (2.0 * decimation);
    if (!(cutoff <= rate / 2.0)) usage_error("--cutoff must be in [0, rate / 2]");
    if (hop == 0) hop = fft_size;

    FILE *fp = fopen(path, "rb");
    if (fp == NULL) {
        fprintf(stderr, "fsea-zoom-fft: cannot open recording %s\n", path);
        return EXIT_FAILURE;
    }
    fseek(fp, 0L, SEEK_END);
    const long size = ftell(fp);
    rewind(fp);
    const size_t n_samples = size > 0 ? (size_t)size / 2 : 0;
    uint8_t *iq = (uint8_t *)malloc(n_samples > 0 ? 2 * n_samples : 1);
    if (iq == NULL) usage_error("out of memory");
    if (fread(iq, 1, 2 * n_samples, fp) != 2 * n_samples) {
        fprintf(stderr, "fsea-zoom-fft: cannot read recording %s\n", path);
        return EXIT_FAILURE;
    }
    fclose(fp);

    double *c = (double *)malloc(sizeof(double) * (size_t)taps);
    if (c == NULL) usage_error("out of memory");
    if (fsea_fir_lowpass_taps(rate, cutoff, taps, c) != FSEA_OK) die("fsea_fir_lowpass_taps");
    fsea_zoom *zoom = NULL;
    if (fsea_zoom_create(&zoom, c, taps, decimation, fft_size, hop, FSEA_MODE_DB10_U8, 0) != FSEA_OK) die("fsea_zoom_create");
    free(c);
    const size_t rows = fsea_zoom_out_rows(zoom, n_samples);
    if (rows < 1) {
        fprintf(stderr, "fsea-zoom-fft: recording %s holds %zu samples, fewer than one row of %d x %d\n", path, n_samples,
                decimation, fft_size);
        return EXIT_FAILURE;
    }
    if (rows > 0x7fffffffu / (size_t)fft_size) usage_error("the image would hold more than 2^31 pixels");
    uint8_t *image = (uint8_t *)malloc(rows * fsea_zoom_row_bytes(zoom));
    if (image == NULL) usage_error("out of memory");
    if (fsea_zoom_run_host(zoom, iq, n_samples, 1, offset / rate, 0.0, 0, image, NULL) != FSEA_OK) die("fsea_zoom_run_host");
    fsea_zoom_destroy(zoom);
    free(iq);
    printf("rows %zu\nbin width %.6f Hz\n", rows, rate / ((double)decimation * (double)fft_size));
    if (write_gray_png(out, fft_size, (int)rows, image) != 0) {
        fprintf(stderr, "fsea-zoom-fft: cannot write %s\n", out);
        return EXIT_FAILURE;
    }
    free(image);
    return 0;
}
