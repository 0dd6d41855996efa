/*
 * fsea-events -- which emissions a recording or a spectrum image holds: one time-frequency box per burst.
 *
 * fsea-occupancy says which columns are occupied how often; this tool says which emissions there were.  It takes
 * fsea-occupancy's inputs and detector: a raw 8-bit IQ recording read in chunks, every frame of N samples (a frame every H)
 * through a plan in a dB mode, the rows given to a fsea_cfar object with a mask, all on the device; or, with --image IN.png,
 * the rows of an 8-bit grey PNG.  The mask and the rows under it then go to a fsea_events object (include/fsea.h), which
 * reduces them to runs; the tool keeps all runs of the input on the host and links them once at the end into events: the
 * connected components of runs that touch across up to --gap-cols free columns and --gap-rows free rows.  Events lower than
 * --min-rows, narrower than --min-cols or with fewer than --min-hits detections are dropped.  It prints
 *     rows R runs N events E
 * and one line per event: row_first row_last col_first col_last hits peak peak_row peak_col.  With --rate and --freq the three
 * columns follow as MHz by fsea-occupancy's formula, column k of N being FREQ + (k - N / 2) * RATE / N; for a recording the
 * three rows then follow as seconds, row r beginning r * H / RATE into it.  --paint OUT.png writes the runs of the surviving
 * events, closed gaps included, as a mask of one row per frame: 255 inside, 0 elsewhere.
 *
 * usage: fsea-events FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db] [--guard G] [--train T]
 *                    [--offset LEVELS] [--method ca|go|so] [--gap-cols B] [--gap-rows R] [--min-rows R] [--min-cols B]
 *                    [--min-hits K] [--rate HZ --freq MHZ] [--paint OUT.png]
 *        fsea-events --image IN.png [the detector's and the events' options]
 */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

static const char *USAGE =
    "usage: fsea-events FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db] [--guard G] [--train T]\n"
    "                   [--offset LEVELS] [--method ca|go|so] [--gap-cols B] [--gap-rows R] [--min-rows R] [--min-cols B]\n"
    "                   [--min-hits K] [--rate HZ --freq MHZ] [--paint OUT.png]\n"
    "       fsea-events --image IN.png [--guard G] ... [--paint OUT.png]\n"
    "  FILE is a raw 8-bit IQ recording (--flip: HackRF int8); every frame of N samples, one every H, becomes a dB row on the\n"
    "  GPU and fsea-occupancy's CFAR detector (--guard, --train, --offset, --method; --mode db: f32 dB rows, LEVELS in 1/64 dB)\n"
    "  marks the bins that hold a signal; --image IN.png scans the rows of an 8-bit grey PNG instead.  Detections of a row\n"
    "  with at most --gap-cols free bins between them are a run; runs at most --gap-rows free rows apart that overlap, give\n"
    "  or take --gap-cols bins, belong to one event.  Events lower than --min-rows rows, narrower than --min-cols bins or of\n"
    "  fewer than --min-hits detections are dropped.  Prints `rows R runs N events E` and per event\n"
    "  `row_first row_last col_first col_last hits peak peak_row peak_col`, with --rate and --freq also the columns as MHz\n"
    "  and, for a recording, the rows as seconds; --paint OUT.png writes the surviving events as a mask\n"
    "  defaults: --hop N --window rect --mode db5 --guard 2 --train 16 --offset 60 --method ca --gap-cols 0 --gap-rows 0\n"
    "  --min-rows 1 --min-cols 1 --min-hits 1";

static void usage_error(const char *msg) { tool_usage_error("fsea-events", msg); }

static void die(const char *what) { tool_die("fsea-events", what); }

/* all runs of the input, in order */
static fsea_events_run *g_runs = NULL;
static size_t g_n_runs = 0, g_cap_runs = 0;

static fsea_events_run *runs_room(size_t more) {
    if (g_n_runs + more > g_cap_runs) {
        size_t cap = g_cap_runs ? g_cap_runs : 1024;
        while (cap < g_n_runs + more) cap *= 2;
        fsea_events_run *grown = (fsea_events_run *)realloc(g_runs, cap * sizeof(fsea_events_run));
        if (grown == NULL) usage_error("out of memory");
        g_runs = grown;
        g_cap_runs = cap;
    }
    return g_runs + g_n_runs;
}

int main(int argc, char **argv) {
    const char *path = NULL, *paint_path = NULL, *window = "rect", *mode_name = "db5";
    int size = 0, hop = 0, flip = 0, gap_cols = 0, gap_rows = 0;
    long long min_rows = 1, min_cols = 1, min_hits = 1;
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
        else if (tool_detector_option("fsea-events", &det, argc, argv, &i)) continue;
        else if (!strcmp(argv[i], "--gap-cols") && more) gap_cols = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gap-rows") && more) gap_rows = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--min-rows") && more) min_rows = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-cols") && more) min_cols = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-hits") && more) min_hits = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--paint") && more) paint_path = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    const char *image_path = det.image_path;
    const double rate = det.rate, freq = det.freq;
    if (path == NULL && image_path == NULL) usage_error("no recording file given");
    if (path != NULL && image_path != NULL) usage_error("a recording or --image, not both");
    if (image_path == NULL && (size < 1 || size > FSEA_EVENTS_MAX_WIDTH)) usage_error("--size must be in [1, 1048576]");
    if (hop == 0) hop = size;
    if (image_path == NULL && hop < 1) usage_error("--hop must be positive");
    tool_detector_check("fsea-events", &det);
    if (gap_cols < 0 || gap_cols > FSEA_EVENTS_MAX_GAP_COLS) usage_error("--gap-cols must be in [0, 64]");
    if (gap_rows < 0 || gap_rows > FSEA_EVENTS_MAX_GAP_ROWS) usage_error("--gap-rows must be in [0, 65536]");
    if (min_rows < 1 || min_rows > 0xffffffffll) usage_error("--min-rows must be at least 1");
    if (min_cols < 1 || min_cols > 0xffffffffll) usage_error("--min-cols must be at least 1");
    if (min_hits < 1) usage_error("--min-hits must be at least 1");
    tool_detector_check_axis("fsea-events", &det);
    int mode = 0, type = 0;
    if (!tool_rows_mode(mode_name, "db", &mode, &type)) usage_error("--mode must be db5, db10 or db");

    /* The object counts the rows of every call; the tool counts its own (`done`) and has the object start each chunk at row
     * 0, so that a chunk can be asked twice: once for the number of its runs, once for the records. */
    fsea_cfar *cfar = NULL;
    fsea_events *events = NULL;
    int width = size;
    size_t done = 0;
    if (image_path != NULL) {
        int height = 0;
        uint8_t *image = tool_detector_image("fsea-events", &det, &width, &height, &cfar);
        if (fsea_events_create(&events, width, 0) != FSEA_OK) die("fsea_events_create");
        if (fsea_events_set_gap(events, gap_cols) != FSEA_OK) die("fsea_events_set_gap");
        uint8_t *mask = (uint8_t *)malloc((size_t)width * (size_t)height + 1);
        if (mask == NULL) usage_error("out of memory");
        const size_t h = (size_t)height, w = (size_t)width;
        if (fsea_cfar_add_host(cfar, image, FSEA_CFAR_U8, h, w, mask, NULL) != FSEA_OK) die("fsea_cfar_add_host");
        size_t found = 0;
        if (fsea_events_runs_host(events, mask, w, image, FSEA_CFAR_U8, w, h, NULL, 0, &found) != FSEA_OK) die("fsea_events_runs_host");
        if (fsea_events_reset(events) != FSEA_OK) die("fsea_events_reset");
        if (fsea_events_runs_host(events, mask, w, image, FSEA_CFAR_U8, w, h, runs_room(found), found, &found) != FSEA_OK) {
            die("fsea_events_runs_host");
        }
        g_n_runs = found;
        done = h;
        free(mask);
        free(image);
    } else {
        tool_row_source src;
        tool_rows_open(&src, "fsea-events", path, size, hop, mode, window, flip);
        cfar = tool_detector_create("fsea-events", &det, size);
        if (fsea_events_create(&events, size, 0) != FSEA_OK) die("fsea_events_create");
        if (fsea_events_set_gap(events, gap_cols) != FSEA_OK) die("fsea_events_set_gap");
        const size_t n = (size_t)size;
        void *d_rows = src.d_rows, *d_mask = NULL, *d_runs = NULL;
        size_t d_runs_cap = 0;
        if (fsea_device_alloc(0, src.frames_max * n, &d_mask) != FSEA_OK) die("fsea_device_alloc");
        /* rows and mask stay on the device between the plan, the detector and the runs; everything on the null stream */
        for (size_t frames; (frames = tool_rows_next(&src)) > 0; done += frames) {
            if (fsea_cfar_add_device(cfar, d_rows, type, frames, n, (uint8_t *)d_mask, NULL, NULL) != FSEA_OK) die("fsea_cfar_add_device");
            size_t found = 0;
            if (fsea_events_reset(events) != FSEA_OK) die("fsea_events_reset");
            if (fsea_events_runs_device(events, (const uint8_t *)d_mask, n, d_rows, type, n, frames, NULL, 0, &found, NULL) != FSEA_OK) {
                die("fsea_events_runs_device");
            }
            if (found > 0) {
                if (found > d_runs_cap) {
                    if (d_runs != NULL) fsea_device_free(0, d_runs);
                    d_runs_cap = found + found / 2;
                    if (fsea_device_alloc(0, d_runs_cap * sizeof(fsea_events_run), &d_runs) != FSEA_OK) die("fsea_device_alloc");
                }
                if (fsea_events_reset(events) != FSEA_OK) die("fsea_events_reset");
                if (fsea_events_runs_device(events, (const uint8_t *)d_mask, n, d_rows, type, n, frames, (fsea_events_run *)d_runs, found,
                                            &found, NULL) != FSEA_OK) {
                    die("fsea_events_runs_device");
                }
                fsea_events_run *dst = runs_room(found);
                if (fsea_copy_to_host(0, dst, d_runs, found * sizeof(fsea_events_run)) != FSEA_OK) die("fsea_copy_to_host");
                if (done + frames > 0xffffffffull) usage_error("the recording holds more than 2^32 - 1 frames");
                for (size_t i = 0; i < found; i++) dst[i].row += (uint32_t)done;
                g_n_runs += found;
            }
        }
        tool_rows_close(&src);
        fsea_device_free(0, d_mask);
        if (d_runs != NULL) fsea_device_free(0, d_runs);
    }
    if (done < 1) {
        if (image_path != NULL) fprintf(stderr, "fsea-events: image %s has no rows\n", image_path);
        else return tool_rows_none("fsea-events", path, size);
        return EXIT_FAILURE;
    }

    /* one link over all runs of the input */
    uint32_t *event_of_run = (uint32_t *)malloc(sizeof(uint32_t) * (g_n_runs + 1));
    if (event_of_run == NULL) usage_error("out of memory");
    size_t n_events = 0;
    if (fsea_events_link(g_runs, g_n_runs, gap_cols, gap_rows, (uint32_t)min_rows, (uint32_t)min_cols, (uint64_t)min_hits, NULL, NULL, 0,
                         &n_events) != FSEA_OK) {
        die("fsea_events_link");
    }
    fsea_events_event *found_events = (fsea_events_event *)malloc(sizeof(fsea_events_event) * (n_events + 1));
    if (found_events == NULL) usage_error("out of memory");
    if (fsea_events_link(g_runs, g_n_runs, gap_cols, gap_rows, (uint32_t)min_rows, (uint32_t)min_cols, (uint64_t)min_hits, event_of_run,
                         found_events, n_events, &n_events) != FSEA_OK) {
        die("fsea_events_link");
    }
    printf("rows %zu runs %zu events %zu\n", done, g_n_runs, n_events);
    for (size_t j = 0; j < n_events; j++) {
        const fsea_events_event *e = &found_events[j];
        printf("%u %u %u %u %llu %d %u %u", e->row_first, e->row_last, e->col_first, e->col_last, (unsigned long long)e->hits, e->peak,
               e->peak_row, e->peak_col);
        if (rate > 0.0) {
            const uint32_t k[3] = {e->col_first, e->col_last, e->peak_col}, r[3] = {e->row_first, e->row_last, e->peak_row};
            for (int i = 0; i < 3; i++) printf(" %.6f", tool_column_mhz(freq, rate, width, k[i]));
            if (image_path == NULL) {
                for (int i = 0; i < 3; i++) printf(" %.6f", (double)r[i] * (double)hop / rate);
            }
        }
        putchar('\n');
    }
    if (paint_path != NULL) {
        if (done > (size_t)INT_MAX) usage_error("too many rows for a PNG");
        uint8_t *values = (uint8_t *)malloc(g_n_runs + 1), *image = (uint8_t *)malloc(done * (size_t)width + 1);
        if (values == NULL || image == NULL) usage_error("out of memory");
        for (size_t i = 0; i < g_n_runs; i++) values[i] = event_of_run[i] != FSEA_EVENTS_NO_EVENT ? 255 : 0;
        if (fsea_events_paint_host(events, g_runs, values, g_n_runs, 0, done, image, (size_t)width) != FSEA_OK) die("fsea_events_paint_host");
        if (write_gray_png(paint_path, width, (int)done, image) != 0) {
            fprintf(stderr, "fsea-events: cannot write %s\n", paint_path);
            return EXIT_FAILURE;
        }
        free(values);
        free(image);
    }
    fsea_events_destroy(events);
    fsea_cfar_destroy(cfar);
    free(found_events);
    free(event_of_run);
    free(g_runs);
    return 0;
}
