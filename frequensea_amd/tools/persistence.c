/*
 * fsea-persistence -- the persistence spectrum of a recording: how often each of N bins was at each of 256 levels.
 *
 * The reference's spectrum tools write one row per frame (c/fft-batch.c); an analyser's persistence display is the
 * histogram of those rows per bin.  This one reads a raw 8-bit IQ recording in chunks, runs every frame of N samples
 * (a frame every H) through a plan in a dB mode (include/fsea.h) and adds the rows, still on the device, to a fsea_persist
 * object.  The 256 x N picture, strongest level on top, goes to an 8-bit grey PNG through write_gray_png; the rows counted
 * and the occupied level range are printed.  --traces FILE writes one line per column: column, max-hold level, median
 * level, lowest level.
 *
 * usage: fsea-persistence FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db:LO:HI] [--map sat|lin|log]
 *                         [--full COUNT] [--traces FILE] -o OUT.png
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"
#include "tool_common.h"

static const char *USAGE =
    "usage: fsea-persistence FILE --size N [--hop H] [--window NAME] [--flip] [--mode db5|db10|db:LO:HI] [--map sat|lin|log]\n"
    "                        [--full COUNT] [--traces FILE] -o OUT.png\n"
    "  FILE is a raw 8-bit IQ recording (--flip: HackRF int8); every frame of N samples, one every H, becomes a dB row on the\n"
    "  GPU and is counted there: the 256 x N picture says how often each bin was at each level, the strongest level on top;\n"
    "  --mode db:LO:HI counts f32 dB rows over the range [LO, HI); --full COUNT is the count shown as white (default: the rows);\n"
    "  --traces FILE writes `column max quantile50 min` per column\n"
    "  defaults: --hop N --window rect --mode db5 --map log -o persistence.png";

static void usage_error(const char *msg) { tool_usage_error("fsea-persistence", msg); }

static void die(const char *what) { tool_die("fsea-persistence", what); }

int main(int argc, char **argv) {
    const char *out = "persistence.png", *path = NULL, *traces_path = NULL, *window = "rect", *mode_name = "db5";
    int size = 0, hop = 0, flip = 0, map = FSEA_PERSIST_MAP_LOG;
    unsigned long long full = 0;
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
        else if (!strcmp(argv[i], "--map") && more) {
            const char *m = argv[++i];
            if (!strcmp(m, "sat")) map = FSEA_PERSIST_MAP_SATURATE;
            else if (!strcmp(m, "lin")) map = FSEA_PERSIST_MAP_LINEAR;
            else if (!strcmp(m, "log")) map = FSEA_PERSIST_MAP_LOG;
            else usage_error("--map must be sat, lin or log");
        } else if (!strcmp(argv[i], "--full") && more) full = strtoull(argv[++i], NULL, 10);
        else if (!strcmp(argv[i], "--traces") && more) traces_path = argv[++i];
        else if ((!strcmp(argv[i], "-o") || !strcmp(argv[i], "--out")) && more) out = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    if (path == NULL) usage_error("no recording file given");
    if (size < 1 || size > FSEA_PERSIST_MAX_WIDTH) usage_error("--size must be in [1, 65536]");
    if (hop == 0) hop = size;
    if (hop < 1) usage_error("--hop must be positive");
    int mode = FSEA_MODE_DB_F32, type = FSEA_PERSIST_F32;
    float lo = 0.0f, hi = 0.0f;
    if (!strncmp(mode_name, "db:", 3)) {
        if (sscanf(mode_name + 3, "%f:%f", &lo, &hi) != 2 || !isfinite(lo) || !isfinite(hi) || !(lo < hi)) {
            usage_error("--mode db:LO:HI needs two finite numbers with LO < HI");
        }
    } else if (!tool_rows_mode(mode_name, NULL, &mode, &type)) usage_error("--mode must be db5, db10 or db:LO:HI");

    tool_row_source src;
    tool_rows_open(&src, "fsea-persistence", path, size, hop, mode, window, flip);
    fsea_persist *persist = NULL;
    if (fsea_persist_create(&persist, size, 0) != FSEA_OK) die("fsea_persist_create");
    if (type == FSEA_PERSIST_F32 && fsea_persist_set_range(persist, lo, hi) != FSEA_OK) die("fsea_persist_set_range");
    /* the rows stay on the device between the plan and the object */
    const size_t n = (size_t)size;
    for (size_t frames; (frames = tool_rows_next(&src)) > 0;) {
        if (fsea_persist_add_device(persist, src.d_rows, type, frames, n, NULL) != FSEA_OK) die("fsea_persist_add_device");
    }
    tool_rows_close(&src);
    const unsigned long long rows = fsea_persist_rows(persist);
    if (rows < 1) return tool_rows_none("fsea-persistence", path, size);

    uint8_t *image = (uint8_t *)malloc((size_t)FSEA_PERSIST_LEVELS * n);
    uint32_t *counts = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)FSEA_PERSIST_LEVELS * n);
    uint8_t *trace = (uint8_t *)malloc(3 * n);
    if (image == NULL || counts == NULL || trace == NULL) usage_error("out of memory");
    if (fsea_persist_image_host(persist, map, full, image) != FSEA_OK) die("fsea_persist_image_host");
    if (fsea_persist_counts_host(persist, counts) != FSEA_OK) die("fsea_persist_counts_host");
    if (fsea_persist_trace(counts, size, FSEA_PERSIST_TRACE_MAX, 0.0, trace) != FSEA_OK ||
        fsea_persist_trace(counts, size, FSEA_PERSIST_TRACE_QUANTILE, 0.5, trace + n) != FSEA_OK ||
        fsea_persist_trace(counts, size, FSEA_PERSIST_TRACE_MIN, 0.0, trace + 2 * n) != FSEA_OK) die("fsea_persist_trace");
    int level_lo = 255, level_hi = 0;
    for (size_t k = 0; k < n; k++) {
        if (trace[k] > level_hi) level_hi = trace[k];
        if (trace[2 * n + k] < level_lo) level_lo = trace[2 * n + k];
    }
    printf("rows %llu\nlevels %d to %d\n", rows, level_lo, level_hi);
    if (write_gray_png(out, size, FSEA_PERSIST_LEVELS, image) != 0) {
        fprintf(stderr, "fsea-persistence: cannot write %s\n", out);
        return EXIT_FAILURE;
    }
    if (traces_path != NULL) {
        FILE *tp = fopen(traces_path, "w");
        if (tp == NULL) {
            fprintf(stderr, "fsea-persistence: cannot write %s\n", traces_path);
            return EXIT_FAILURE;
        }
        for (size_t k = 0; k < n; k++) fprintf(tp, "%zu %d %d %d\n", k, trace[k], trace[n + k], trace[2 * n + k]);
        if (fclose(tp) != 0) {
            fprintf(stderr, "fsea-persistence: cannot write %s\n", traces_path);
            return EXIT_FAILURE;
        }
    }
    fsea_persist_destroy(persist);
    free(trace);
    free(counts);
    free(image);
    return 0;
}
