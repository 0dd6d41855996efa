/*
 * nrf_private.h -- what the files of the host library share beside the public headers: the fatal-error convention, checked
 * allocation, device selection and the small buffer plumbing of the nrf blocks.
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
