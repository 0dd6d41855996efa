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
 * events, closed gaps included, as a mask of one row per frame: 255 inside, 0 elsewhere.  --axis time and --axis either are
 * fsea-occupancy's: the detector down the time axis (fsea_tcfar), alone or OR-ed into the frequency detector's mask.
 *
 * usage: fsea-events FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db] [--guard G] [--train T]
 *                    [--offset LEVELS] [--method ca|go|so | --rank R] [--axis freq|time|either] [--gap-cols B] [--gap-rows R]
 *                    [--min-rows R] [--min-cols B] [--min-hits K] [--rate HZ --freq MHZ] [--paint OUT.png]
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
    "                   [--offset LEVELS] [--method ca|go|so] [--rank R] [--axis freq|time|either] [--gap-cols B]\n"
    "                   [--gap-rows R] [--min-rows R] [--min-cols B] [--min-hits K] [--rate HZ --freq MHZ] [--paint OUT.png]\n"
    "       fsea-events --image IN.png [--guard G] ... [--paint OUT.png]\n"
    "  FILE is a raw 8-bit IQ recording (--flip: HackRF int8); every frame of N samples, one every H, becomes a dB row on the\n"
    "  GPU and fsea-occupancy's CFAR detector (--guard, --train, --offset, --method; --mode db: f32 dB rows, LEVELS in 1/64 dB;\n"
    "  --rank R in place of --method: its ordered-statistic detector, the R-th smallest of the 2 T bins in place of their mean;\n"
    "  --axis time: a bin against the same bin of the T frames before and after it; --axis either: both, OR-ed)\n"
    "  marks the bins that hold a signal; --image IN.png scans the rows of an 8-bit grey PNG instead.  Detections of a row\n"
    "  with at most --gap-cols free bins between them are a run; runs at most --gap-rows free rows apart that overlap, give\n"
    "  or take --gap-cols bins, belong to one event.  Events lower than --min-rows rows, narrower than --min-cols bins or of\n"
    "  fewer than --min-hits detections are dropped.  Prints `rows R runs N events E` and per event\n"
    "  `row_first row_last col_first col_last hits peak peak_row peak_col`, with --rate and --freq also the columns as MHz\n"
    "  and, for a recording, the rows as seconds; --paint OUT.png writes the surviving events as a mask\n"
    "  defaults: --hop N --window rect --mode db5 --guard 2 --train 16 --offset 60 --method ca --axis freq --gap-cols 0 --gap-rows 0\n"
    "  --min-rows 1 --min-cols 1 --min-hits 1";

static void usage_error(const char *msg) { tool_usage_error("fsea-events", msg); }

static void die(const char *what) { tool_die("fsea-events", what); }

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

    tool_detector_object detector = {NULL, NULL, NULL};
    fsea_events *events = NULL;
    tool_run_list list = {NULL, 0, 0};   /* all runs of the input, in order */
    int width = size;
    size_t done = 0;
    if (image_path != NULL) {
        int height = 0;
        uint8_t *image = tool_detector_image("fsea-events", &det, &width, &height, &detector);
        if (fsea_events_create(&events, width, 0) != FSEA_OK) die("fsea_events_create");
        if (fsea_events_set_gap(events, gap_cols) != FSEA_OK) die("fsea_events_set_gap");
        uint8_t *mask = (uint8_t *)malloc((size_t)width * (size_t)height + 1);
        if (mask == NULL) usage_error("out of memory");
        const size_t h = (size_t)height, w = (size_t)width;
        tool_detector_add_host("fsea-events", &detector, image, FSEA_CFAR_U8, h, w, mask);
        size_t found = 0;
        if (fsea_events_runs_host(events, mask, w, image, FSEA_CFAR_U8, w, h, NULL, 0, &found) != FSEA_OK) die("fsea_events_runs_host");
        if (fsea_events_reset(events) != FSEA_OK) die("fsea_events_reset");
        fsea_events_run *dst = tool_runs_room("fsea-events", &list, found);
        if (fsea_events_runs_host(events, mask, w, image, FSEA_CFAR_U8, w, h, dst, found, &found) != FSEA_OK) die("fsea_events_runs_host");
        list.n = found;
        done = h;
        free(mask);
        free(image);
    } else {
        tool_row_source src;
        tool_detector_check_chunk("fsea-events", &det, size, hop, type);
        tool_rows_open(&src, "fsea-events", path, size, hop, mode, window, flip);
        tool_rows_keep(&src, tool_detector_keep(&det, size, type));
        detector = tool_detector_create("fsea-events", &det, size);
        if (fsea_events_create(&events, size, 0) != FSEA_OK) die("fsea_events_create");
        if (fsea_events_set_gap(events, gap_cols) != FSEA_OK) die("fsea_events_set_gap");
        done = tool_recording_runs("fsea-events", &src, &detector, events, type, &list);
        tool_rows_close(&src);
    }
    if (done < 1) {
        if (image_path != NULL) fprintf(stderr, "fsea-events: image %s has no rows\n", image_path);
        else return tool_rows_none("fsea-events", path, size);
        return EXIT_FAILURE;
    }

    /* one link over all runs of the input */
    uint32_t *event_of_run = (uint32_t *)malloc(sizeof(uint32_t) * (list.n + 1));
    if (event_of_run == NULL) usage_error("out of memory");
    size_t n_events = 0;
    fsea_events_event *found_events = tool_link("fsea-events", &list, gap_cols, gap_rows, min_rows, min_cols, min_hits, event_of_run, &n_events);
    printf("rows %zu runs %zu events %zu\n", done, list.n, n_events);
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
        uint8_t *values = (uint8_t *)malloc(list.n + 1), *image = (uint8_t *)malloc(done * (size_t)width + 1);
        if (values == NULL || image == NULL) usage_error("out of memory");
        for (size_t i = 0; i < list.n; i++) values[i] = event_of_run[i] != FSEA_EVENTS_NO_EVENT ? 255 : 0;
        if (fsea_events_paint_host(events, list.runs, values, list.n, 0, done, image, (size_t)width) != FSEA_OK) die("fsea_events_paint_host");
        if (write_gray_png(paint_path, width, (int)done, image) != 0) {
            fprintf(stderr, "fsea-events: cannot write %s\n", paint_path);
            return EXIT_FAILURE;
        }
        free(values);
        free(image);
    }
    fsea_events_destroy(events);
    tool_detector_destroy(&detector);
    free(found_events);
    free(event_of_run);
    free(list.runs);
    return 0;
}
