/*
 * tool_common.h -- what the command-line tools share beside pipeline.h (which stays about threads and rings): the two ways a
 * tool ends with a message, the capture format's constants, the newest-first row reader of the sweep tools, the --window
 * names, and what the tools that give dB rows to a device object share (fsea-persistence, fsea-occupancy, fsea-events): the
 * recording that becomes rows on the device chunk by chunk (chunks that overlap where a detector down the time axis needs
 * context rows), the --mode names, the CFAR detectors' options (--axis among them) and the MHz of a column; and for fsea-events and fsea-cutouts the list of an input's runs, its filling from a recording and the link into
 * events; a device buffer with its pinned twin, regrown by half.  All `static inline`, as in pipeline.h; a tool takes its part.
 *
 * The --window table is the tools' own: the host library keeps one like it in its private header, which no tool includes.
 */
#ifndef FSEA_TOOLS_TOOL_COMMON_H
#define FSEA_TOOLS_TOOL_COMMON_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "easypng.h"
#include "fsea.h"

#define TRANSFER_BYTES 262144 /* one HackRF transfer: 131072 IQ samples, as c/rfcap.c records them */
#define EVALUATE_ROWS 100     /* c/fft-batch-broad.c:22 */

/* a failed library call: the tool, what it was doing, the library's own text */
static inline void tool_die(const char *tool, const char *what) {
    fprintf(stderr, "%s: %s: %s\n", tool, what, fsea_last_error_string());
    exit(EXIT_FAILURE);
}

/* a wrong command line, or anything else the tool can say in one line */
static inline void tool_usage_error(const char *tool, const char *msg) {
    fprintf(stderr, "%s: %s\n", tool, msg);
    exit(EXIT_FAILURE);
}

/* A device buffer and, where asked for, its pinned twin on the host, regrown by half when a call needs more; zeroed to begin
 * with.  What they held is gone after a regrowth. */
typedef struct {
    void *d, *h;
    size_t cap; /* elements */
} tool_grown;

static inline void tool_grown_free(tool_grown *g) {
    if (g->d != NULL) fsea_device_free(0, g->d);
    if (g->h != NULL) fsea_host_free(g->h);
    memset(g, 0, sizeof(*g));
}

static inline void tool_grown_need(const char *tool, tool_grown *g, size_t count, size_t elem_bytes, int pinned) {
    if (count <= g->cap) return;
    tool_grown_free(g);
    g->cap = count + count / 2;
    if (fsea_device_alloc(0, g->cap * elem_bytes, &g->d) != FSEA_OK) tool_die(tool, "fsea_device_alloc");
    if (pinned && fsea_host_alloc(g->cap * elem_bytes, &g->h) != FSEA_OK) tool_die(tool, "fsea_host_alloc");
}

/* --window NAME: the periodic cosine-sum taper of that name on the plan (include/fsea.h: fsea_window_fill; the position in
 * the table is the kind).  0, a failure of the library (or of malloc), or TOOL_WINDOW_UNKNOWN: the caller words that one. */
#define TOOL_WINDOW_UNKNOWN (-2)
/* the kind of a --window name (FSEA_WINDOW_*), or TOOL_WINDOW_UNKNOWN */
static inline int tool_window_kind(const char *name) {
    static const char *names[] = {"rect", "hann", "hamming", "blackman", "blackmanharris", "flattop"};
    for (int k = 0; k < 6; k++) {
        if (strcmp(name, names[k]) == 0) return k;
    }
    return TOOL_WINDOW_UNKNOWN;
}

static inline int tool_set_named_window(fsea_plan *plan, const char *name, int n) {
    const int k = tool_window_kind(name);
    if (k == TOOL_WINDOW_UNKNOWN) return k;
    float *w = (float *)malloc(sizeof(float) * (size_t)n);
    if (!w) return -1;
    int rc = fsea_window_fill(k, n, w);
    if (rc == 0 && k != 0) rc = fsea_plan_set_window(plan, w);
    free(w);
    return rc;
}

/* --mode NAME of the tools that give rows to an object: db5 and db10 are 8-bit rows; `f32_name` ("db"; NULL: the tool has
 * a form of its own) is f32 dB rows.  The type is FSEA_CFAR_U8 / _F32, which FSEA_PERSIST_U8 / _F32 equal.  0: no such name. */
static inline int tool_rows_mode(const char *name, const char *f32_name, int *mode, int *type) {
    *type = FSEA_CFAR_U8;
    if (!strcmp(name, "db5")) *mode = FSEA_MODE_DB5_U8_DCFIX;
    else if (!strcmp(name, "db10")) *mode = FSEA_MODE_DB10_U8;
    else if (f32_name != NULL && !strcmp(name, f32_name)) {
        *mode = FSEA_MODE_DB_F32;
        *type = FSEA_CFAR_F32;
    } else return 0;
    return 1;
}

/* column k of `width` as MHz: the plan's rows have the centre frequency, `freq` MHz, in column width / 2 */
static inline double tool_column_mhz(double freq, double rate, int width, long long k) {
    return freq + (double)(k - width / 2) * rate / (double)width / 1e6;
}

/* A raw 8-bit IQ recording as dB rows on the device: every frame of n samples, one every h, through a plan with the named
 * window, in chunks of whole frames of at most TOOL_CHUNK_SAMPLES samples and TOOL_CHUNK_ROW_BYTES of rows, one frame at
 * least.  The rows of a chunk are in d_rows, n to a row, until the next chunk is asked for; everything on the null stream,
 * in order.  With `keep` > 0 (tool_rows_keep, for a detector down the time axis) consecutive chunks overlap by 2 * keep
 * frames: rows lo .. hi - 1 of a chunk are its own, the `keep` rows before and behind them are context and belong to the
 * neighbouring chunks, so every row of the recording is some chunk's own exactly once, with `keep` rows of context on each
 * side wherever the recording has them.  Without it lo = 0 and hi = the frames of the chunk. */
#define TOOL_CHUNK_SAMPLES ((size_t)1 << 22)
#define TOOL_CHUNK_ROW_BYTES ((size_t)256 << 20)

/* the frames of a chunk at most, for rows of row_bytes */
static inline size_t tool_chunk_frames(size_t n, size_t h, size_t row_bytes) {
    size_t frames_max = TOOL_CHUNK_ROW_BYTES / row_bytes;
    if (TOOL_CHUNK_SAMPLES > n && (TOOL_CHUNK_SAMPLES - n) / h + 1 < frames_max) frames_max = (TOOL_CHUNK_SAMPLES - n) / h + 1;
    if (frames_max < 1 || TOOL_CHUNK_SAMPLES <= n) frames_max = 1;
    return frames_max;
}
typedef struct {
    const char *tool;
    FILE *fp;
    fsea_plan *plan;
    int flip;
    size_t n, h, chunk, frames_max;   /* samples and frames of a chunk at most */
    long long pos;                    /* the sample the next chunk begins at */
    size_t keep, total, first;        /* context rows each side; frames of the recording; the frame the next chunk begins at */
    size_t lo, hi;                    /* the chunk's own rows */
    uint8_t *iq;
    void *d_iq, *d_rows;
} tool_row_source;

/* "cannot open recording" comes before any device call; every failure ends the tool */
static inline void tool_rows_open(tool_row_source *s, const char *tool, const char *path, int size, int hop, int mode,
                                  const char *window, int flip) {
    memset(s, 0, sizeof(*s));
    s->tool = tool;
    s->flip = flip;
    s->fp = fopen(path, "rb");
    if (s->fp == NULL) {
        fprintf(stderr, "%s: cannot open recording %s\n", tool, path);
        exit(EXIT_FAILURE);
    }
    if (fsea_plan_create(&s->plan, size, hop, mode, 0) != FSEA_OK) tool_die(tool, "fsea_plan_create");
    const int wrc = tool_set_named_window(s->plan, window, size);
    if (wrc == TOOL_WINDOW_UNKNOWN) tool_usage_error(tool, "--window must be rect, hann, hamming, blackman, blackmanharris or flattop");
    if (wrc != 0) tool_die(tool, "--window");
    const size_t n = (size_t)size, h = (size_t)hop, row_bytes = fsea_plan_row_bytes(s->plan);
    const size_t frames_max = tool_chunk_frames(n, h, row_bytes);
    s->n = n;
    s->h = h;
    s->frames_max = frames_max;
    s->chunk = (frames_max - 1) * h + n;
    s->iq = (uint8_t *)malloc(2 * s->chunk);
    if (s->iq == NULL) tool_usage_error(tool, "out of memory");
    if (fsea_device_alloc(0, 2 * s->chunk, &s->d_iq) != FSEA_OK) tool_die(tool, "fsea_device_alloc");
    if (fsea_device_alloc(0, frames_max * row_bytes, &s->d_rows) != FSEA_OK) tool_die(tool, "fsea_device_alloc");
}

/* Chunks of the opened source overlap by 2 * keep frames from here on (before the first tool_rows_next); the caller has
 * checked that a chunk holds 2 * keep + 1 frames (tool_detector_check_chunk). */
static inline void tool_rows_keep(tool_row_source *s, size_t keep) {
    s->keep = keep;
    s->total = 0;
    if (fseek(s->fp, 0, SEEK_END) == 0) {
        const long long samples = (long long)ftell(s->fp) / 2;
        if (samples >= (long long)s->n) s->total = (size_t)((samples - (long long)s->n) / (long long)s->h) + 1;
    }
}

/* the frames of the next chunk, now in d_rows, lo and hi set; 0: the recording holds no further frame */
static inline size_t tool_rows_next(tool_row_source *s) {
    if (fseek(s->fp, 2 * s->pos, SEEK_SET) != 0) return 0;
    const size_t got = fread(s->iq, 2, s->chunk, s->fp);
    if (got < s->n) return 0;
    const size_t frames = (got - s->n) / s->h + 1;
    if (fsea_copy_to_device(0, s->d_iq, s->iq, 2 * got) != FSEA_OK) tool_die(s->tool, "fsea_copy_to_device");
    if (fsea_exec_u8_device(s->plan, s->d_iq, frames, s->flip, s->d_rows, NULL) != FSEA_OK) tool_die(s->tool, "fsea_exec_u8_device");
    /* the last chunk of an overlapping walk keeps its tail; every other gives its last 2 * keep frames to the next as well */
    const int last = s->keep == 0 || s->first + frames >= s->total;
    s->lo = s->first == 0 ? 0 : s->keep;
    s->hi = last ? frames : frames - s->keep;
    const size_t step = last ? frames : frames - 2 * s->keep;
    s->first += step;
    s->pos += (long long)(step * s->h);
    return frames;
}

static inline void tool_rows_close(tool_row_source *s) {
    fclose(s->fp);
    fsea_plan_destroy(s->plan);
    fsea_device_free(0, s->d_iq);
    fsea_device_free(0, s->d_rows);
    free(s->iq);
}

/* what a tool says of a recording that gave no row, for its exit status */
static inline int tool_rows_none(const char *tool, const char *path, int size) {
    fprintf(stderr, "%s: recording %s holds fewer than one frame of %d samples\n", tool, path, size);
    return EXIT_FAILURE;
}

/* The CFAR detector of fsea-occupancy, fsea-events and fsea-cutouts: --guard --train --offset --method, or --rank R in place
 * of --method for the ordered-statistic detector (fsea_oscfar); --axis freq|time|either: across frequency (the default), down
 * the time axis (fsea_tcfar, --guard and --train counted in rows), or the frequency detector exactly as given and fsea_tcfar
 * with the same guard, train, offset and method OR-ed into its mask; the axis of --rate and --freq, and --image IN.png in
 * place of a recording. */
enum { TOOL_AXIS_FREQ = 0, TOOL_AXIS_TIME = 1, TOOL_AXIS_EITHER = 2 };
typedef struct {
    int guard, train, offset, method, have_freq;
    double rate, freq;
    const char *image_path;
    int rank, have_rank, have_method;
    int axis;
} tool_detector;
#define TOOL_DETECTOR_DEFAULTS {2, 16, 60, FSEA_CFAR_CA, 0, 0.0, 0.0, NULL, 0, 0, 0, TOOL_AXIS_FREQ}

/* 1: argv[*i] was one of the detector's options and *i is on its value; 0: not one of them */
static inline int tool_detector_option(const char *tool, tool_detector *d, int argc, char **argv, int *i) {
    const char *arg = argv[*i];
    if (*i + 1 >= argc) return 0;
    if (!strcmp(arg, "--guard")) d->guard = atoi(argv[++*i]);
    else if (!strcmp(arg, "--train")) d->train = atoi(argv[++*i]);
    else if (!strcmp(arg, "--offset")) d->offset = atoi(argv[++*i]);
    else if (!strcmp(arg, "--method")) {
        const char *m = argv[++*i];
        if (!strcmp(m, "ca")) d->method = FSEA_CFAR_CA;
        else if (!strcmp(m, "go")) d->method = FSEA_CFAR_GO;
        else if (!strcmp(m, "so")) d->method = FSEA_CFAR_SO;
        else tool_usage_error(tool, "--method must be ca, go or so");
        d->have_method = 1;
    } else if (!strcmp(arg, "--rank")) {
        d->rank = atoi(argv[++*i]);
        d->have_rank = 1;
    } else if (!strcmp(arg, "--axis")) {
        const char *a = argv[++*i];
        if (!strcmp(a, "freq")) d->axis = TOOL_AXIS_FREQ;
        else if (!strcmp(a, "time")) d->axis = TOOL_AXIS_TIME;
        else if (!strcmp(a, "either")) d->axis = TOOL_AXIS_EITHER;
        else tool_usage_error(tool, "--axis must be freq, time or either");
    } else if (!strcmp(arg, "--rate")) d->rate = atof(argv[++*i]);
    else if (!strcmp(arg, "--freq")) {
        d->freq = atof(argv[++*i]);
        d->have_freq = 1;
    } else if (!strcmp(arg, "--image")) d->image_path = argv[++*i];
    else return 0;
    return 1;
}

/* the ranges of the detector's own; a tool checks --rate and --freq behind its own options */
static inline void tool_detector_check(const char *tool, const tool_detector *d) {
    if (d->guard < 0 || d->guard > FSEA_CFAR_MAX_GUARD) tool_usage_error(tool, "--guard must be in [0, 64]");
    if (d->train < 1 || d->train > FSEA_CFAR_MAX_TRAIN) tool_usage_error(tool, "--train must be in [1, 256]");
    if (d->offset < -FSEA_CFAR_MAX_OFFSET || d->offset > FSEA_CFAR_MAX_OFFSET) {
        tool_usage_error(tool, "--offset must be in [-1048576, 1048576]");
    }
    if (d->have_rank && d->have_method) tool_usage_error(tool, "--rank R is a detector of its own: not together with --method");
    if (d->have_rank && (d->rank < 1 || d->rank > 2 * d->train)) tool_usage_error(tool, "--rank must be in [1, 2 * --train]");
    if (d->have_rank && d->axis == TOOL_AXIS_TIME) tool_usage_error(tool, "--rank R is across frequency: not together with --axis time");
}

/* The context rows a chunk of a recording keeps on each side of its own rows: 0 across frequency; down the time axis G + T,
 * or the next count at which the chunk's own rows begin at a 16-byte boundary, as the device forms ask. */
static inline size_t tool_detector_keep(const tool_detector *d, int size, int type) {
    if (d->axis == TOOL_AXIS_FREQ) return 0;
    size_t keep = (size_t)(d->guard + d->train);
    const size_t row_bytes = (size_t)size * (type == FSEA_CFAR_F32 ? 4 : 1);
    while (keep * row_bytes % 16 != 0) keep++;
    return keep;
}

/* a recording down the time axis: a chunk of frames of `size` samples every `hop` holds a row of its own between its context
 * rows, or the command line is wrong; before any device call */
static inline void tool_detector_check_chunk(const char *tool, const tool_detector *d, int size, int hop, int type) {
    const size_t keep = tool_detector_keep(d, size, type);
    const size_t frames = tool_chunk_frames((size_t)size, (size_t)hop, (size_t)size * (type == FSEA_CFAR_F32 ? 4 : 1));
    if (keep > 0 && frames < 2 * keep + 1) {
        fprintf(stderr, "%s: a chunk holds %zu frames, and --guard %d --train %d down the time axis need %zu\n", tool, frames, d->guard,
                d->train, 2 * keep + 1);
        exit(EXIT_FAILURE);
    }
}

static inline void tool_detector_check_axis(const char *tool, const tool_detector *d) {
    if ((d->rate != 0.0) != d->have_freq || d->rate < 0.0) tool_usage_error(tool, "--rate HZ (positive) and --freq MHZ go together");
}

/* The tool's detector: a fsea_cfar, or with --rank a fsea_oscfar; with --axis time a fsea_tcfar in their place, with --axis
 * either a fsea_tcfar behind one of them, which ORs its decisions into their mask.  Their add, rows and hits forms have the
 * same arguments but the context rows, so a tool names the set and these pass the call on, with the entry point's name for
 * tool_die.  Where there is a fsea_tcfar it is the last to write the mask, so rows and hits are its own. */
typedef struct {
    fsea_cfar *cfar;
    fsea_oscfar *oscfar;
    fsea_tcfar *tcfar;
} tool_detector_object;

/* a detector of `width` columns with the options' settings */
static inline tool_detector_object tool_detector_create(const char *tool, const tool_detector *d, int width) {
    tool_detector_object o = {NULL, NULL, NULL};
    if (d->axis != TOOL_AXIS_FREQ) {
        const int op = d->axis == TOOL_AXIS_EITHER ? FSEA_TCFAR_MASK_OR : FSEA_TCFAR_MASK_SET;
        if (fsea_tcfar_create(&o.tcfar, width, 0) != FSEA_OK) tool_die(tool, "fsea_tcfar_create");
        if (fsea_tcfar_set(o.tcfar, d->guard, d->train, d->offset, d->method, op) != FSEA_OK) tool_die(tool, "fsea_tcfar_set");
        if (d->axis == TOOL_AXIS_TIME) return o;
    }
    if (d->have_rank) {
        if (fsea_oscfar_create(&o.oscfar, width, 0) != FSEA_OK) tool_die(tool, "fsea_oscfar_create");
        if (fsea_oscfar_set(o.oscfar, d->guard, d->train, d->offset, d->rank) != FSEA_OK) tool_die(tool, "fsea_oscfar_set");
        return o;
    }
    if (fsea_cfar_create(&o.cfar, width, 0) != FSEA_OK) tool_die(tool, "fsea_cfar_create");
    if (fsea_cfar_set(o.cfar, d->guard, d->train, d->offset, d->method) != FSEA_OK) tool_die(tool, "fsea_cfar_set");
    return o;
}

/* whether the detector cannot do without a mask: the frequency detector's, which the fsea_tcfar behind it reads */
static inline int tool_detector_needs_mask(const tool_detector_object *o) { return o->tcfar != NULL && (o->cfar != NULL || o->oscfar != NULL); }

/* n_rows rows from d_rows on, `before` context rows in front of them and `after` behind (read down the time axis only) */
static inline void tool_detector_add_device(const char *tool, const tool_detector_object *o, const void *d_rows, int type, size_t n_rows,
                                            size_t pitch, size_t before, size_t after, uint8_t *d_mask) {
    if (o->oscfar != NULL) {
        if (fsea_oscfar_add_device(o->oscfar, d_rows, type, n_rows, pitch, d_mask, NULL, NULL) != FSEA_OK) tool_die(tool, "fsea_oscfar_add_device");
    } else if (o->cfar != NULL) {
        if (fsea_cfar_add_device(o->cfar, d_rows, type, n_rows, pitch, d_mask, NULL, NULL) != FSEA_OK) tool_die(tool, "fsea_cfar_add_device");
    }
    if (o->tcfar != NULL && fsea_tcfar_add_device(o->tcfar, d_rows, type, n_rows, pitch, before, after, d_mask, NULL, NULL) != FSEA_OK) {
        tool_die(tool, "fsea_tcfar_add_device");
    }
}

/* the whole of an input in one call: no context */
static inline void tool_detector_add_host(const char *tool, const tool_detector_object *o, const void *rows, int type, size_t n_rows,
                                          size_t pitch, uint8_t *mask) {
    if (o->oscfar != NULL) {
        if (fsea_oscfar_add_host(o->oscfar, rows, type, n_rows, pitch, mask, NULL) != FSEA_OK) tool_die(tool, "fsea_oscfar_add_host");
    } else if (o->cfar != NULL) {
        if (fsea_cfar_add_host(o->cfar, rows, type, n_rows, pitch, mask, NULL) != FSEA_OK) tool_die(tool, "fsea_cfar_add_host");
    }
    if (o->tcfar != NULL && fsea_tcfar_add_host(o->tcfar, rows, type, n_rows, pitch, 0, 0, mask, NULL) != FSEA_OK) {
        tool_die(tool, "fsea_tcfar_add_host");
    }
}

/* the own rows of the source's current chunk (tool_rows_next) with their context, mask row 0 at d_mask */
static inline void tool_detector_add_chunk(const char *tool, const tool_detector_object *o, const tool_row_source *src, size_t frames,
                                           int type, uint8_t *d_mask) {
    const char *own = (const char *)src->d_rows + src->lo * src->n * (type == FSEA_CFAR_F32 ? 4 : 1);
    tool_detector_add_device(tool, o, own, type, src->hi - src->lo, src->n, src->lo, frames - src->hi, d_mask);
}

static inline unsigned long long tool_detector_rows(const tool_detector_object *o) {
    if (o->tcfar != NULL) return fsea_tcfar_rows(o->tcfar);
    return o->oscfar != NULL ? fsea_oscfar_rows(o->oscfar) : fsea_cfar_rows(o->cfar);
}

static inline void tool_detector_hits_host(const char *tool, const tool_detector_object *o, uint32_t *hits) {
    if (o->tcfar != NULL) {
        if (fsea_tcfar_hits_host(o->tcfar, hits) != FSEA_OK) tool_die(tool, "fsea_tcfar_hits_host");
    } else if (o->oscfar != NULL) {
        if (fsea_oscfar_hits_host(o->oscfar, hits) != FSEA_OK) tool_die(tool, "fsea_oscfar_hits_host");
    } else if (fsea_cfar_hits_host(o->cfar, hits) != FSEA_OK) tool_die(tool, "fsea_cfar_hits_host");
}

static inline void tool_detector_destroy(tool_detector_object *o) {
    fsea_tcfar_destroy(o->tcfar);
    fsea_oscfar_destroy(o->oscfar);
    fsea_cfar_destroy(o->cfar);
    o->tcfar = NULL;
    o->oscfar = NULL;
    o->cfar = NULL;
}

/* --image: the rows of the PNG (the caller frees them), their size, and a detector of their width */
static inline uint8_t *tool_detector_image(const char *tool, const tool_detector *d, int *width, int *height, tool_detector_object *det) {
    uint8_t *image = read_gray_png(d->image_path, width, height);
    if (image == NULL) {
        fprintf(stderr, "%s: cannot read %s as an 8-bit grey PNG\n", tool, d->image_path);
        exit(EXIT_FAILURE);
    }
    if (*width < 1 || *width > FSEA_CFAR_MAX_WIDTH) tool_usage_error(tool, "the image is wider than 1048576 columns");
    *det = tool_detector_create(tool, d, *width);
    return image;
}

/* All runs of an input, in order (fsea-events, fsea-cutouts): a growing array, zeroed to begin with; the tool frees `runs`. */
typedef struct {
    fsea_events_run *runs;
    size_t n, cap;
} tool_run_list;

/* where `more` runs behind the list's own go; the caller adds what it put there to `n` */
static inline fsea_events_run *tool_runs_room(const char *tool, tool_run_list *list, size_t more) {
    if (list->n + more > list->cap) {
        size_t cap = list->cap ? list->cap : 1024;
        while (cap < list->n + more) cap *= 2;
        fsea_events_run *grown = (fsea_events_run *)realloc(list->runs, cap * sizeof(fsea_events_run));
        if (grown == NULL) tool_usage_error(tool, "out of memory");
        list->runs = grown;
        list->cap = cap;
    }
    return list->runs + list->n;
}

/* The runs of a recording, to the list: the own rows of every chunk of the opened `src` to the detector with a mask, mask and
 * rows (of `type`) to the events object, on the device and the null stream.  The object starts each chunk at row 0, so that a
 * chunk can be asked twice: for the number of its runs, then for the records, whose rows this rebases.  Returns the rows done. */
static inline size_t tool_recording_runs(const char *tool, tool_row_source *src, const tool_detector_object *det, fsea_events *events,
                                         int type, tool_run_list *list) {
    const size_t n = src->n;
    void *d_rows = src->d_rows, *d_mask = NULL;
    tool_grown d_runs = {NULL, NULL, 0};
    size_t done = 0;
    if (fsea_device_alloc(0, src->frames_max * n, &d_mask) != FSEA_OK) tool_die(tool, "fsea_device_alloc");
    for (size_t chunk, frames = 0; (chunk = tool_rows_next(src)) > 0; done += frames) {
        tool_detector_add_chunk(tool, det, src, chunk, type, (uint8_t *)d_mask);
        frames = src->hi - src->lo;
        d_rows = (char *)src->d_rows + src->lo * n * (type == FSEA_CFAR_F32 ? 4 : 1);
        size_t found = 0;
        if (fsea_events_reset(events) != FSEA_OK) tool_die(tool, "fsea_events_reset");
        if (fsea_events_runs_device(events, (const uint8_t *)d_mask, n, d_rows, type, n, frames, NULL, 0, &found, NULL) != FSEA_OK) {
            tool_die(tool, "fsea_events_runs_device");
        }
        if (found == 0) continue;
        tool_grown_need(tool, &d_runs, found, sizeof(fsea_events_run), 0);
        if (fsea_events_reset(events) != FSEA_OK) tool_die(tool, "fsea_events_reset");
        if (fsea_events_runs_device(events, (const uint8_t *)d_mask, n, d_rows, type, n, frames, (fsea_events_run *)d_runs.d, found, &found,
                                    NULL) != FSEA_OK) {
            tool_die(tool, "fsea_events_runs_device");
        }
        fsea_events_run *dst = tool_runs_room(tool, list, found);
        if (fsea_copy_to_host(0, dst, d_runs.d, found * sizeof(fsea_events_run)) != FSEA_OK) tool_die(tool, "fsea_copy_to_host");
        if (done + frames > 0xffffffffull) tool_usage_error(tool, "the recording holds more than 2^32 - 1 frames");
        for (size_t i = 0; i < found; i++) dst[i].row += (uint32_t)done;
        list->n += found;
    }
    fsea_device_free(0, d_mask);
    tool_grown_free(&d_runs);
    return done;
}

/* One link over all runs of the input with the tool's checked --gap-cols, --gap-rows, --min-rows, --min-cols and --min-hits:
 * the number of events, then the events themselves (the caller frees them).  event_of_run: NULL, or room for an entry per run. */
static inline fsea_events_event *tool_link(const char *tool, const tool_run_list *list, int gap_cols, int gap_rows, long long min_rows,
                                           long long min_cols, long long min_hits, uint32_t *event_of_run, size_t *n_events) {
    const uint32_t rows = (uint32_t)min_rows, cols = (uint32_t)min_cols;
    int rc = fsea_events_link(list->runs, list->n, gap_cols, gap_rows, rows, cols, (uint64_t)min_hits, NULL, NULL, 0, n_events);
    if (rc != FSEA_OK) tool_die(tool, "fsea_events_link");
    fsea_events_event *found = (fsea_events_event *)malloc(sizeof(fsea_events_event) * (*n_events + 1));
    if (found == NULL) tool_usage_error(tool, "out of memory");
    rc = fsea_events_link(list->runs, list->n, gap_cols, gap_rows, rows, cols, (uint64_t)min_hits, event_of_run, found, *n_events, n_events);
    if (rc != FSEA_OK) tool_die(tool, "fsea_events_link");
    return found;
}

#if defined(_POSIX_C_SOURCE) && _POSIX_C_SOURCE >= 200809L /* pread: the sweep tools are built with it */
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

/* Rows of one capture, newest first: row y <- first 2N bytes of transfer skip + rows - 1 - y (c/fft-batch.c:62-74), up to
 * rows_wanted of them; need_all makes fewer than rows_wanted too few, otherwise only none is.
 * 0 = loaded, > 0 = fatal (cannot open, short read), < 0 = too few transfers; every case but 0 has been reported.
 * One pread per row (a row is the first 2N bytes of a 262144-byte transfer): stdio's fseek + fread pair refills its buffer
 * for every row, twice the system calls for the 4.9 million rows of the reference's narrow sweep. */
static inline int tool_load_rows(const char *tool, const char *path, int fft_size, int skip, int rows_wanted, int need_all,
                                 uint8_t *packed, int *rows_out) {
    const size_t row_in = (size_t)2 * (size_t)fft_size;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "%s: cannot open %s\n", tool, path);
        return 1;
    }
    struct stat st;
    if (fstat(fd, &st) != 0) {
        fprintf(stderr, "%s: cannot stat %s\n", tool, path);
        close(fd);
        return 1;
    }
    const long transfers = (long)(st.st_size / TRANSFER_BYTES);
    int rows = (int)(transfers - skip);
    if (rows > rows_wanted) rows = rows_wanted;
    if (need_all ? rows < rows_wanted : rows <= 0) {
        if (need_all) {
            fprintf(stderr, "%s: %s holds %ld transfers, need %d after skipping %d\n", tool, path, transfers, rows_wanted, skip);
        } else {
            fprintf(stderr, "%s: %s holds %ld transfers, need more than %d\n", tool, path, transfers, skip);
        }
        close(fd);
        return -1;
    }
    for (int y = 0; y < rows; y++) {
        const off_t tr = (off_t)skip + rows - 1 - y;
        uint8_t *dst = packed + (size_t)y * row_in;
        size_t got = 0;
        while (got < row_in) {
            const ssize_t r = pread(fd, dst + got, row_in - got, tr * (off_t)TRANSFER_BYTES + (off_t)got);
            if (r <= 0) break;
            got += (size_t)r;
        }
        if (got != row_in) {
            fprintf(stderr, "Short read, samples lost, exiting!\n");
            close(fd);
            return 1;
        }
    }
    close(fd);
    *rows_out = rows;
    return 0;
}
#endif

#endif
