/*
 * fsea-occupancy -- which bins of a recording or of a spectrum image hold a signal, and which bands are occupied how often.
 *
 * The reference's only spectrum-side detector is the 100-row gate of c/fft-batch-broad.c, which keeps or drops a whole centre
 * frequency.  This one reads a raw 8-bit IQ recording in chunks, runs every frame of N samples (a frame every H) through a
 * plan in a dB mode (include/fsea.h) and gives the rows, still on the device, to a fsea_cfar object: a constant-false-alarm-
 * rate detector across frequency.  With --image IN.png the rows are those of an 8-bit grey PNG instead, a stitched sweep for
 * example.  It prints the rows decided and one line per band of occupied columns: first last peak duty, the duty being the
 * share of the rows in which the band's peak column was detected; with --rate and --freq the three columns follow as MHz:
 * column k of N is FREQ + (k - N / 2) * RATE / N, the plan's rows having the centre frequency in column N / 2.  --mask OUT.png
 * writes the detections, one row per frame, 255 for a hit; --bands FILE writes the band lines.
 *
 * usage: fsea-occupancy FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db] [--guard G] [--train T]
 *                       [--offset LEVELS] [--method ca|go|so] [--min-duty F] [--max-gap B] [--min-width B]
 *                       [--rate HZ --freq MHZ] [--mask OUT.png] [--bands FILE]
 *        fsea-occupancy --image IN.png [the detector's and the bands' options]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

#define CHUNK_SAMPLES ((size_t)1 << 22)        /* samples read at a time */
#define CHUNK_ROW_BYTES ((size_t)256 << 20)    /* and the rows of a chunk at most */

static const char *USAGE =
    "usage: fsea-occupancy FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db] [--guard G] [--train T]\n"
    "                      [--offset LEVELS] [--method ca|go|so] [--min-duty F] [--max-gap B] [--min-width B]\n"
    "                      [--rate HZ --freq MHZ] [--mask OUT.png] [--bands FILE]\n"
    "       fsea-occupancy --image IN.png [--guard G] ... [--bands FILE]\n"
    "  FILE is a raw 8-bit IQ recording (--flip: HackRF int8); every frame of N samples, one every H, becomes a dB row on the\n"
    "  GPU and a CFAR detector compares each bin with the mean level of T bins on either side, G guard bins left out:\n"
    "  a bin is detected when its level is more than LEVELS above that mean (--mode db: f32 dB rows, LEVELS in 1/64 dB);\n"
    "  --method go asks that of each side (steps do not fire), so of either side; --image IN.png scans the rows of an 8-bit\n"
    "  grey PNG instead; a bin detected in at least F of the rows is occupied, bands bridge up to --max-gap free bins and are\n"
    "  at least --min-width wide; prints `rows R` and `first last peak duty` per band, with --rate and --freq also as MHz\n"
    "  defaults: --hop N --window rect --mode db5 --guard 2 --train 16 --offset 60 --method ca --min-duty 0.5 --max-gap 0\n"
    "  --min-width 1";

static void usage_error(const char *msg) { tool_usage_error("fsea-occupancy", msg); }

static void die(const char *what) { tool_die("fsea-occupancy", what); }

static void print_bands(FILE *f, const fsea_cfar_band *bands, size_t n_bands, unsigned long long rows, int width, double rate,
                        double freq) {
    for (size_t b = 0; b < n_bands; b++) {
        fprintf(f, "%d %d %d %.6f", bands[b].first, bands[b].last, bands[b].peak, (double)bands[b].peak_hits / (double)rows);
        if (rate > 0.0) {
            const int k[3] = {bands[b].first, bands[b].last, bands[b].peak};
            for (int j = 0; j < 3; j++) fprintf(f, " %.6f", freq + (double)(k[j] - width / 2) * rate / (double)width / 1e6);
        }
        fputc('\n', f);
    }
}

int main(int argc, char **argv) {
    const char *path = NULL, *image_path = NULL, *mask_path = NULL, *bands_path = NULL, *window = "rect", *mode_name = "db5";
    int size = 0, hop = 0, flip = 0, guard = 2, train = 16, offset = 60, method = FSEA_CFAR_CA, max_gap = 0, min_width = 1;
    int have_freq = 0;
    double min_duty = 0.5, rate = 0.0, freq = 0.0;
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--help")) {
            puts(USAGE);
            return 0;
        } else if (!strcmp(argv[i], "--size") && more) size = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--hop") && more) hop = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--window") && more) window = argv[++i];
        else if (!strcmp(argv[i], "--flip")) flip = 1;
        else if (!strcmp(argv[i], "--mode") && more) mode_name = argv[++i];
        else if (!strcmp(argv[i], "--guard") && more) guard = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--train") && more) train = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--offset") && more) offset = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--method") && more) {
            const char *m = argv[++i];
            if (!strcmp(m, "ca")) method = FSEA_CFAR_CA;
            else if (!strcmp(m, "go")) method = FSEA_CFAR_GO;
            else if (!strcmp(m, "so")) method = FSEA_CFAR_SO;
            else usage_error("--method must be ca, go or so");
        } else if (!strcmp(argv[i], "--min-duty") && more) min_duty = atof(argv[++i]);
        else if (!strcmp(argv[i], "--max-gap") && more) max_gap = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--min-width") && more) min_width = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--rate") && more) rate = atof(argv[++i]);
        else if (!strcmp(argv[i], "--freq") && more) {
            freq = atof(argv[++i]);
            have_freq = 1;
        } else if (!strcmp(argv[i], "--image") && more) image_path = argv[++i];
        else if (!strcmp(argv[i], "--mask") && more) mask_path = argv[++i];
        else if (!strcmp(argv[i], "--bands") && more) bands_path = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    if (path == NULL && image_path == NULL) usage_error("no recording file given");
    if (path != NULL && image_path != NULL) usage_error("a recording or --image, not both");
    if (image_path == NULL && (size < 1 || size > FSEA_CFAR_MAX_WIDTH)) usage_error("--size must be in [1, 1048576]");
    if (hop == 0) hop = size;
    if (image_path == NULL && hop < 1) usage_error("--hop must be positive");
    if (guard < 0 || guard > FSEA_CFAR_MAX_GUARD) usage_error("--guard must be in [0, 64]");
    if (train < 1 || train > FSEA_CFAR_MAX_TRAIN) usage_error("--train must be in [1, 256]");
    if (offset < -FSEA_CFAR_MAX_OFFSET || offset > FSEA_CFAR_MAX_OFFSET) usage_error("--offset must be in [-1048576, 1048576]");
    if (!(min_duty >= 0.0 && min_duty <= 1.0)) usage_error("--min-duty must be in [0, 1]");
    if (max_gap < 0) usage_error("--max-gap must not be negative");
    if (min_width < 1) usage_error("--min-width must be at least 1");
    if ((rate != 0.0) != have_freq || rate < 0.0) usage_error("--rate HZ (positive) and --freq MHZ go together");
    int mode = FSEA_MODE_DB5_U8_DCFIX, type = FSEA_CFAR_U8;
    if (!strcmp(mode_name, "db10")) mode = FSEA_MODE_DB10_U8;
    else if (!strcmp(mode_name, "db")) {
        mode = FSEA_MODE_DB_F32;
        type = FSEA_CFAR_F32;
    } else if (strcmp(mode_name, "db5") != 0) usage_error("--mode must be db5, db10 or db");

    fsea_cfar *cfar = NULL;
    uint8_t *mask = NULL;          /* rows x width, grown chunk by chunk; only with --mask */
    int width = size;
    if (image_path != NULL) {
        int height = 0;
        uint8_t *image = read_gray_png(image_path, &width, &height);
        if (image == NULL) {
            fprintf(stderr, "fsea-occupancy: cannot read %s as an 8-bit grey PNG\n", image_path);
            return EXIT_FAILURE;
        }
        if (width < 1 || width > FSEA_CFAR_MAX_WIDTH) usage_error("the image is wider than 1048576 columns");
        if (fsea_cfar_create(&cfar, width, 0) != FSEA_OK) die("fsea_cfar_create");
        if (fsea_cfar_set(cfar, guard, train, offset, method) != FSEA_OK) die("fsea_cfar_set");
        if (mask_path != NULL) {
            mask = (uint8_t *)malloc((size_t)width * (size_t)height + 1);
            if (mask == NULL) usage_error("out of memory");
        }
        if (fsea_cfar_add_host(cfar, image, FSEA_CFAR_U8, (size_t)height, (size_t)width, mask, NULL) != FSEA_OK) die("fsea_cfar_add_host");
        free(image);
    } else {
        FILE *fp = fopen(path, "rb");
        if (fp == NULL) {
            fprintf(stderr, "fsea-occupancy: cannot open recording %s\n", path);
            return EXIT_FAILURE;
        }
        fsea_plan *plan = NULL;
        if (fsea_plan_create(&plan, size, hop, mode, 0) != FSEA_OK) die("fsea_plan_create");
        const int wrc = tool_set_named_window(plan, window, size);
        if (wrc == TOOL_WINDOW_UNKNOWN) usage_error("--window must be rect, hann, hamming, blackman, blackmanharris or flattop");
        if (wrc != 0) die("--window");
        if (fsea_cfar_create(&cfar, size, 0) != FSEA_OK) die("fsea_cfar_create");
        if (fsea_cfar_set(cfar, guard, train, offset, method) != FSEA_OK) die("fsea_cfar_set");

        /* a chunk: whole frames, at most CHUNK_SAMPLES samples and CHUNK_ROW_BYTES of rows, one frame at least */
        const size_t n = (size_t)size, h = (size_t)hop, row_bytes = fsea_plan_row_bytes(plan);
        size_t frames_max = CHUNK_ROW_BYTES / row_bytes;
        if (CHUNK_SAMPLES > n && (CHUNK_SAMPLES - n) / h + 1 < frames_max) frames_max = (CHUNK_SAMPLES - n) / h + 1;
        if (frames_max < 1 || CHUNK_SAMPLES <= n) frames_max = 1;
        const size_t chunk = (frames_max - 1) * h + n;
        uint8_t *iq = (uint8_t *)malloc(2 * chunk);
        if (iq == NULL) usage_error("out of memory");
        void *d_iq = NULL, *d_rows = NULL, *d_mask = NULL;
        if (fsea_device_alloc(0, 2 * chunk, &d_iq) != FSEA_OK) die("fsea_device_alloc");
        if (fsea_device_alloc(0, frames_max * row_bytes, &d_rows) != FSEA_OK) die("fsea_device_alloc");
        if (mask_path != NULL && fsea_device_alloc(0, frames_max * n, &d_mask) != FSEA_OK) die("fsea_device_alloc");
        /* the rows stay on the device between the plan and the object; everything on the null stream, in order */
        size_t done = 0;
        for (long long pos = 0;;) {
            if (fseek(fp, 2 * pos, SEEK_SET) != 0) break;
            const size_t got = fread(iq, 2, chunk, fp);
            if (got < n) break;
            const size_t frames = (got - n) / h + 1;
            if (fsea_copy_to_device(0, d_iq, iq, 2 * got) != FSEA_OK) die("fsea_copy_to_device");
            if (fsea_exec_u8_device(plan, d_iq, frames, flip, d_rows, NULL) != FSEA_OK) die("fsea_exec_u8_device");
            if (fsea_cfar_add_device(cfar, d_rows, type, frames, n, (uint8_t *)d_mask, NULL, NULL) != FSEA_OK) die("fsea_cfar_add_device");
            if (mask_path != NULL) {
                uint8_t *grown = (uint8_t *)realloc(mask, (done + frames) * n);
                if (grown == NULL) usage_error("out of memory");
                mask = grown;
                if (fsea_copy_to_host(0, mask + done * n, d_mask, frames * n) != FSEA_OK) die("fsea_copy_to_host");
            }
            done += frames;
            pos += (long long)(frames * h);
        }
        fclose(fp);
        fsea_plan_destroy(plan);
        fsea_device_free(0, d_iq);
        fsea_device_free(0, d_rows);
        if (d_mask != NULL) fsea_device_free(0, d_mask);
        free(iq);
    }
    const unsigned long long rows = fsea_cfar_rows(cfar);
    if (rows < 1) {
        if (image_path != NULL) fprintf(stderr, "fsea-occupancy: image %s has no rows\n", image_path);
        else fprintf(stderr, "fsea-occupancy: recording %s holds fewer than one frame of %d samples\n", path, size);
        return EXIT_FAILURE;
    }

    uint32_t *hits = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)width);
    if (hits == NULL) usage_error("out of memory");
    if (fsea_cfar_hits_host(cfar, hits) != FSEA_OK) die("fsea_cfar_hits_host");
    size_t n_bands = 0;
    if (fsea_cfar_bands(hits, width, rows, min_duty, max_gap, min_width, NULL, 0, &n_bands) != FSEA_OK) die("fsea_cfar_bands");
    fsea_cfar_band *bands = (fsea_cfar_band *)malloc(sizeof(fsea_cfar_band) * (n_bands + 1));
    if (bands == NULL) usage_error("out of memory");
    if (fsea_cfar_bands(hits, width, rows, min_duty, max_gap, min_width, bands, n_bands, &n_bands) != FSEA_OK) die("fsea_cfar_bands");
    printf("rows %llu\n", rows);
    print_bands(stdout, bands, n_bands, rows, width, rate, freq);
    if (mask_path != NULL && write_gray_png(mask_path, width, (int)rows, mask) != 0) {
        fprintf(stderr, "fsea-occupancy: cannot write %s\n", mask_path);
        return EXIT_FAILURE;
    }
    if (bands_path != NULL) {
        FILE *bp = fopen(bands_path, "w");
        if (bp == NULL) {
            fprintf(stderr, "fsea-occupancy: cannot write %s\n", bands_path);
            return EXIT_FAILURE;
        }
        print_bands(bp, bands, n_bands, rows, width, rate, freq);
        if (fclose(bp) != 0) {
            fprintf(stderr, "fsea-occupancy: cannot write %s\n", bands_path);
            return EXIT_FAILURE;
        }
    }
    fsea_cfar_destroy(cfar);
    free(bands);
    free(hits);
    free(mask);
    return 0;
}
