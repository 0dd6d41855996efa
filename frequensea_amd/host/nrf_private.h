/*
 * nrf_private.h -- what the files of the host library share beside the public headers: the fatal-error convention, checked
 * allocation, device selection, the small buffer plumbing of the nrf blocks, taper windows by name, and the step from a
 * block of samples to dB rows on the device that the spectrum-side blocks (persistence, occupancy) begin with.
 *
 * Form, decided once: every helper is a `static inline` function that needs only libc and include/fsea.h.  nrf_fft.c is also
 * compiled alone into libfsea_nrf_fft.so (-DFSEA_NRF_FFT_ONLY), next to an application's own nut.c / nrf.c:
 * a helper with external linkage would be one more undefined symbol of that library, an inline one is not, and the widening
 * loop stays a plain loop in its caller's translation unit.  The three functions that do have a definition in this library
 * (nut.c, nrf_iq_draw.c) are declared at the end, outside that build.
 */
#ifndef FSEA_NRF_PRIVATE_H
#define FSEA_NRF_PRIVATE_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsea.h"
#include "nut.h"

/* A backend failure: the convention of src/nrf.c:54-78, print and exit.  `block` is the name after "NRF ". */
__attribute__((noreturn)) static inline void nrf_private_fatal(const char *block, const char *what, int rc) {
    fprintf(stderr, "NRF %s fatal error: %s failed (%d): %s\n", block, what, rc, fsea_last_error_string());
    exit(EXIT_FAILURE);
}

__attribute__((noreturn)) static inline void nrf_private_oom(const char *block) {
    fprintf(stderr, "NRF %s fatal error: out of memory\n", block);
    exit(EXIT_FAILURE);
}

/* malloc / calloc that do not return NULL; a request for nothing is a request for one element */
static inline void *nrf_private_malloc(const char *block, size_t bytes) {
    void *p = malloc(bytes > 0 ? bytes : 1);
    if (p == NULL) nrf_private_oom(block);
    return p;
}

static inline void *nrf_private_calloc(const char *block, size_t count, size_t size) {
    void *p = calloc(count > 0 ? count : 1, size);
    if (p == NULL) nrf_private_oom(block);
    return p;
}

/* The GPU the nrf blocks use: NRF_FFT_DEVICE in the environment, 0 without it; the reference has no such
 * notion. */
static inline int nrf_private_device(void) {
    const char *dev_env = getenv("NRF_FFT_DEVICE");
    return dev_env ? atoi(dev_env) : 0;
}

/* the samples of a buffer, whichever type it has */
static inline void *nrf_private_payload(const nut_buffer *buffer) {
    return buffer->type == NUT_BUFFER_U8 ? (void *)buffer->data.u8 : (void *)buffer->data.f64;
}

/* f32 results of the device into the f64 of a nut_buffer */
static inline void nrf_private_widen(double *f64, const float *f32, int n) {
    for (int k = 0; k < n; k++) f64[k] = (double)f32[k];
}

/* The low-pass design of nrf_iq_filter_new / nrf_iq_chain_new / nrf_zoom_fft_new / nrf_fir_get_low_pass_coefficients:
 * `length` taps the caller frees.  The caller has checked the length. */
static inline double *nrf_private_lowpass_taps(const char *block, int sample_rate, int half_ampl_freq, int length) {
    double *taps = (double *)nrf_private_malloc(block, sizeof(double) * (size_t)length);
    const int rc = fsea_fir_lowpass_taps((double)sample_rate, (double)half_ampl_freq, length, taps);
    if (rc != FSEA_OK) nrf_private_fatal(block, "fsea_fir_lowpass_taps", rc);
    return taps;
}

/* The blocks that read 8-bit samples only say so and stop when they are handed an F64 buffer. */
static inline void nrf_private_need_u8(const char *block, const nut_buffer *buffer) {
    if (buffer->type == NUT_BUFFER_U8) return;
    fprintf(stderr, "NRF %s fatal error: the block takes 8-bit samples, not an F64 buffer\n", block);
    exit(EXIT_FAILURE);
}

/* Taper names -> fsea_window_fill kinds; -1 = rectangular (no taper: NULL, "", "rect", "none"), -2 = unknown */
static inline int nrf_private_window_kind(const char *name) {
    static const struct { const char *name; int kind; } tapers[] = {
        {"hann", FSEA_WINDOW_HANN},           {"hamming", FSEA_WINDOW_HAMMING}, {"blackman", FSEA_WINDOW_BLACKMAN},
        {"blackmanharris", FSEA_WINDOW_BLACKMANHARRIS}, {"flattop", FSEA_WINDOW_FLATTOP}};
    if (name == NULL || name[0] == '\0' || strcmp(name, "rect") == 0 || strcmp(name, "none") == 0) return -1;
    for (size_t i = 0; i < sizeof(tapers) / sizeof(tapers[0]); i++) {
        if (strcmp(name, tapers[i].name) == 0) return tapers[i].kind;
    }
    return -2;
}

/* X_set_window(name) of a block, before it takes its mutex: a name that is no taper is a programming error in the scene,
 * handled as src/main.cpp handles a wrong argument type: say it and stop.  `entry` is the entry point's name. */
static inline void nrf_private_check_window_name(const char *block, const char *entry, const char *name) {
    if (nrf_private_window_kind(name) != -2) return;
    fprintf(stderr, "NRF %s fatal error: %s: \"%s\" is not one of hann, hamming, blackman, blackmanharris, flattop, rect\n", block,
            entry, name);
    exit(EXIT_FAILURE);
}

/* The named taper (checked by the caller) on a plan of `fft_size` points, or none.  `who`, where not NULL, is added to the
 * fatal line of a taper the plan refuses (a size without a kernel of its own): said loudly, not ignored. */
static inline void nrf_private_set_window(const char *block, const char *who, fsea_plan *plan, int fft_size, const char *name) {
    const int kind = nrf_private_window_kind(name);
    int rc;
    if (kind == -1) {
        rc = fsea_plan_set_window(plan, NULL);
        if (rc != FSEA_OK) nrf_private_fatal(block, "fsea_plan_set_window", rc);
        return;
    }
    float *w = (float *)nrf_private_malloc(block, sizeof(float) * (size_t)fft_size);
    rc = fsea_window_fill(kind, fft_size, w);
    if (rc != FSEA_OK) nrf_private_fatal(block, "fsea_window_fill", rc);
    rc = fsea_plan_set_window(plan, w);
    if (rc != FSEA_OK) {
        char what[96] = "fsea_plan_set_window";
        if (who != NULL) snprintf(what, sizeof(what), "fsea_plan_set_window (%s)", who);
        nrf_private_fatal(block, what, rc);
    }
    free(w);
}

/* device memory of a block that only grows: at least `need` bytes behind *d_ptr, the old contents gone */
static inline void nrf_private_grow(const char *block, int device, void **d_ptr, size_t *cap, size_t need) {
    if (*cap >= need) return;
    int rc = *d_ptr != NULL ? fsea_device_free(device, *d_ptr) : FSEA_OK;
    if (rc != FSEA_OK) nrf_private_fatal(block, "fsea_device_free", rc);
    *d_ptr = NULL;
    *cap = 0;
    rc = fsea_device_alloc(device, need, d_ptr);
    if (rc != FSEA_OK) nrf_private_fatal(block, "fsea_device_alloc", rc);
    *cap = need;
}

/* A block of 8-bit samples to the dB rows of its frames (a FSEA_MODE_DB5_U8_DCFIX plan of n points every `hop` samples)
 * in *d_rows, through *d_iq, both grown as needed; returns the frames, 0 for a block shorter than one.  Everything on the
 * null stream, in order; u8 / 256 with no flip: nrf_device_get_samples_buffer's bytes are offset binary already. */
static inline size_t nrf_private_rows_on_device(const char *block, int device, fsea_plan *plan, size_t n, size_t hop,
                                                const nut_buffer *buffer, void **d_iq, size_t *iq_cap, void **d_rows,
                                                size_t *rows_cap) {
    const size_t length = (size_t)buffer->length;
    if (length < n) return 0;
    const size_t frames = (length - n) / hop + 1;
    nrf_private_grow(block, device, d_iq, iq_cap, 2 * length);
    nrf_private_grow(block, device, d_rows, rows_cap, frames * n);
    int rc = fsea_copy_to_device(device, *d_iq, buffer->data.u8, 2 * length);
    if (rc != FSEA_OK) nrf_private_fatal(block, "fsea_copy_to_device", rc);
    rc = fsea_exec_u8_device(plan, *d_iq, frames, 0, *d_rows, NULL);
    if (rc != FSEA_OK) nrf_private_fatal(block, "fsea_exec_u8_device", rc);
    return frames;
}

#ifdef FSEA_NRF_FFT_ONLY
/* only the public nut.h interface is available */
#define nut_private_new_f64_unfilled(n_elements, n_channels) nut_buffer_new_f64((n_elements), (n_channels), NULL)
#else
/* nut.c: F64 buffer (length x channels) whose payload is NOT zero-filled, for callers that overwrite every element at once
 * (nrf_fft_get_buffer linearising its ring). */
nut_buffer *nut_private_new_f64_unfilled(int n_elements, int n_channels);

/* nrf_iq_draw.c, shared with nrf_iq_chain.c: the points nrf_buffer_to_iq_lines joins for a buffer of `size` elements and a
 * line_percentage (the reference's clamp and float product), and its print-and-exit check of a size_multiplier. */
int nrf_private_iq_line_points(int size, float line_percentage);
void nrf_private_check_iq_multiplier(int size_multiplier);
#endif

#endif
