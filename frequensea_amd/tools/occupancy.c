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
 * writes the detections, one row per frame, 255 for a hit; --bands FILE writes the band lines.  --axis time puts the
 * detector's question down each column instead (fsea_tcfar: a bin against the same bin in the frames before and after it,
 * --guard and --train counted in frames), --axis either detects across frequency as given and ORs the time axis in.
 *
 * usage: fsea-occupancy FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db] [--guard G] [--train T]
 *                       [--offset LEVELS] [--method ca|go|so | --rank R] [--axis freq|time|either] [--min-duty F] [--max-gap B]
 *                       [--min-width B] [--rate HZ --freq MHZ] [--mask OUT.png] [--bands FILE]
 *        fsea-occupancy --image IN.png [the detector's and the bands' options]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

static const char *USAGE =
    "usage: fsea-occupancy FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db] [--guard G] [--train T]\n"
    "                      [--offset LEVELS] [--method ca|go|so] [--rank R] [--axis freq|time|either] [--min-duty F]\n"
    "                      [--max-gap B] [--min-width B] [--rate HZ --freq MHZ] [--mask OUT.png] [--bands FILE]\n"
    "       fsea-occupancy --image IN.png [--guard G] ... [--bands FILE]\n"
    "  FILE is a raw 8-bit IQ recording (--flip: HackRF int8); every frame of N samples, one every H, becomes a dB row on the\n"
    "  GPU and a CFAR detector compares each bin with the mean level of T bins on either side, G guard bins left out:\n"
    "  a bin is detected when its level is more than LEVELS above that mean (--mode db: f32 dB rows, LEVELS in 1/64 dB);\n"
    "  --method go asks that of each side (steps do not fire), so of either side; --rank R, in place of --method, compares\n"
    "  with the R-th smallest of the 2 T bins (R in [1, 2 T]; 24 of 32: the weaker of two close signals keeps its bins)\n"
    "  in place of the mean; --axis time compares a bin with the same bin of the T frames before and after it instead, G\n"
    "  frames left out (a burst wider than any window; not with --rank), --axis either detects across frequency as given\n"
    "  and adds what --axis time finds with the same G, T, LEVELS and method; --image IN.png scans the rows of an 8-bit\n"
    "  grey PNG instead; a bin detected in at least F of the rows is occupied, bands bridge up to --max-gap free bins and are\n"
    "  at least --min-width wide; prints `rows R` and `first last peak duty` per band, with --rate and --freq also as MHz\n"
    "  defaults: --hop N --window rect --mode db5 --guard 2 --train 16 --offset 60 --method ca --axis freq --min-duty 0.5 --max-gap 0\n"
    "  --min-width 1";

static void usage_error(const char *msg) { tool_usage_error("fsea-occupancy", msg); }

static void die(const char *what) { tool_die("fsea-occupancy", what); }

static void print_bands(FILE *f, const fsea_cfar_band *bands, size_t n_bands, unsigned long long rows, int width, double rate,
                        double freq) {
    for (size_t b = 0; b < n_bands; b++) {
        fprintf(f, "%d %d %d %.6f", bands[b].first, bands[b].last, bands[b].peak, (double)bands[b].peak_hits / (double)rows);
        if (rate > 0.0) {
            const int k[3] = {bands[b].first, bands[b].last, bands[b].peak};
            for (int j = 0; j < 3; j++) fprintf(f, " %.6f", tool_column_mhz(freq, rate, width, k[j]));
        }
        fputc('\n', f);
    }
}

int main(int argc, char **argv) {
    const char *path = NULL, *mask_path = NULL, *bands_path = NULL, *window = "rect", *mode_name = "db5";
    int size = 0, hop = 0, flip = 0, max_gap = 0, min_width = 1;
    double min_duty = 0.5;
    tool_detector det = TOOL_DETECTOR_DEFAULTS;
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
        else if (tool_detector_option("fsea-occupancy", &det, argc, argv, &i)) continue;
        else if (!strcmp(argv[i], "--min-duty") && more) min_duty = atof(argv[++i]);
        else if (!strcmp(argv[i], "--max-gap") && more) max_gap = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--min-width") && more) min_width = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--mask") && more) mask_path = argv[++i];
        else if (!strcmp(argv[i], "--bands") && more) bands_path = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    const char *image_path = det.image_path;
    if (path == NULL && image_path == NULL) usage_error("no recording file given");
    if (path != NULL && image_path != NULL) usage_error("a recording or --image, not both");
    if (image_path == NULL && (size < 1 || size > FSEA_CFAR_MAX_WIDTH)) usage_error("--size must be in [1, 1048576]");
    if (hop == 0) hop = size;
    if (image_path == NULL && hop < 1) usage_error("--hop must be positive");
    tool_detector_check("fsea-occupancy", &det);
    if (!(min_duty >= 0.0 && min_duty <= 1.0)) usage_error("--min-duty must be in [0, 1]");
    if (max_gap < 0) usage_error("--max-gap must not be negative");
    if (min_width < 1) usage_error("--min-width must be at least 1");
    tool_detector_check_axis("fsea-occupancy", &det);
    int mode = 0, type = 0;
    if (!tool_rows_mode(mode_name, "db", &mode, &type)) usage_error("--mode must be db5, db10 or db");

    tool_detector_object detector = {NULL, NULL, NULL};
    uint8_t *mask = NULL;          /* rows x width, grown chunk by chunk; only with --mask */
    const int with_mask = mask_path != NULL || det.axis == TOOL_AXIS_EITHER;   /* either: the second detector reads the first's */
    int width = size;
    if (image_path != NULL) {
        int height = 0;
        uint8_t *image = tool_detector_image("fsea-occupancy", &det, &width, &height, &detector);
        if (with_mask) {
            mask = (uint8_t *)malloc((size_t)width * (size_t)height + 1);
            if (mask == NULL) usage_error("out of memory");
        }
        tool_detector_add_host("fsea-occupancy", &detector, image, FSEA_CFAR_U8, (size_t)height, (size_t)width, mask);
        free(image);
    } else {
        tool_row_source src;
        tool_detector_check_chunk("fsea-occupancy", &det, size, hop, type);
        tool_rows_open(&src, "fsea-occupancy", path, size, hop, mode, window, flip);
        tool_rows_keep(&src, tool_detector_keep(&det, size, type));
        detector = tool_detector_create("fsea-occupancy", &det, size);
        const size_t n = (size_t)size;
        void *d_mask = NULL;
        if (with_mask && fsea_device_alloc(0, src.frames_max * n, &d_mask) != FSEA_OK) die("fsea_device_alloc");
        /* the rows stay on the device between the plan and the object */
        size_t done = 0;
        for (size_t chunk, frames = 0; (chunk = tool_rows_next(&src)) > 0; done += frames) {
            tool_detector_add_chunk("fsea-occupancy", &detector, &src, chunk, type, (uint8_t *)d_mask);
            frames = src.hi - src.lo;          /* the chunk's own rows */
            if (mask_path != NULL) {
                uint8_t *grown = (uint8_t *)realloc(mask, (done + frames) * n);
                if (grown == NULL) usage_error("out of memory");
                mask = grown;
                if (fsea_copy_to_host(0, mask + done * n, d_mask, frames * n) != FSEA_OK) die("fsea_copy_to_host");
            }
        }
        tool_rows_close(&src);
        if (d_mask != NULL) fsea_device_free(0, d_mask);
    }
    const unsigned long long rows = tool_detector_rows(&detector);
    if (rows < 1) {
        if (image_path != NULL) fprintf(stderr, "fsea-occupancy: image %s has no rows\n", image_path);
        else return tool_rows_none("fsea-occupancy", path, size);
        return EXIT_FAILURE;
    }

    uint32_t *hits = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)width);
    if (hits == NULL) usage_error("out of memory");
    tool_detector_hits_host("fsea-occupancy", &detector, hits);
    size_t n_bands = 0;
    if (fsea_cfar_bands(hits, width, rows, min_duty, max_gap, min_width, NULL, 0, &n_bands) != FSEA_OK) die("fsea_cfar_bands");
    fsea_cfar_band *bands = (fsea_cfar_band *)malloc(sizeof(fsea_cfar_band) * (n_bands + 1));
    if (bands == NULL) usage_error("out of memory");
    if (fsea_cfar_bands(hits, width, rows, min_duty, max_gap, min_width, bands, n_bands, &n_bands) != FSEA_OK) die("fsea_cfar_bands");
    printf("rows %llu\n", rows);
    print_bands(stdout, bands, n_bands, rows, width, det.rate, det.freq);
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
        print_bands(bp, bands, n_bands, rows, width, det.rate, det.freq);
        if (fclose(bp) != 0) {
            fprintf(stderr, "fsea-occupancy: cannot write %s\n", bands_path);
            return EXIT_FAILURE;
        }
    }
    tool_detector_destroy(&detector);
    free(bands);
    free(hits);
    free(mask);
    return 0;
}
