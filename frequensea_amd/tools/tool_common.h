/*
 * tool_common.h -- what the command-line tools share beside pipeline.h (which stays about threads and rings): the two ways a
 * tool ends with a message, the capture format's constants, the newest-first row reader of the sweep tools and the --window
 * names.  Everything is `static inline`, as in pipeline.h; a tool takes what applies to it.
 */
#ifndef FSEA_TOOLS_TOOL_COMMON_H
#define FSEA_TOOLS_TOOL_COMMON_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

/* --window NAME: the periodic cosine-sum taper of that name on the plan (include/fsea.h: fsea_window_fill; the position in
 * the table is the kind).  0, a failure of the library (or of malloc), or TOOL_WINDOW_UNKNOWN: the caller words that one. */
#define TOOL_WINDOW_UNKNOWN (-2)
static inline int tool_set_named_window(fsea_plan *plan, const char *name, int n) {
    static const char *names[] = {"rect", "hann", "hamming", "blackman", "blackmanharris", "flattop"};
    for (int k = 0; k < 6; k++) {
        if (strcmp(name, names[k]) != 0) continue;
        float *w = (float *)malloc(sizeof(float) * (size_t)n);
        if (!w) return -1;
        int rc = fsea_window_fill(k, n, w);
        if (rc == 0 && k != 0) rc = fsea_plan_set_window(plan, w);
        free(w);
        return rc;
    }
    return TOOL_WINDOW_UNKNOWN;
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
