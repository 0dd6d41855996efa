/*
 * nrf_iq_filter.c -- frequensea's FIR filter and IQ low-pass filter blocks (include/nrf.h).
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:654-775.
 *   nrf_fir_get_low_pass_coefficients, nrf_fir_filter_*  host arithmetic in double, as in the reference; the design is
 *                       fsea_fir_lowpass_taps (include/fsea.h), which both this file and the GPU filter use
 *   nrf_iq_filter_*     the convolution of every sample of a block on the GPU (fsea_fir_*: f32, one launch per process
 *                       call); the reference computes it lazily in nrf_iq_filter_get_buffer, here process computes it and
 *                       get_buffer widens a copy to f64 -- the same observable sequence
 * Differences: a kernel length outside [1, FSEA_FIR_MAX_TAPS] prints and exits (the reference would index out of its
 * arrays for < 1), and a mutex serialises process / get_buffer as in nrf_fft.c.
 */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "IQ filter"

/* ---- FIR filter (host, double) ---------------------------------------------- */

double *nrf_fir_get_low_pass_coefficients(int sample_rate, int half_ampl_freq, int length) {
    const int m = length + (length + 1) % 2;
    if (m < 1) {
        fprintf(stderr, "NRF FIR fatal error: filter length %d\n", length);
        exit(EXIT_FAILURE);
    }
    /* m is odd, so the design of length m is all m taps */
    return nrf_private_lowpass_taps(BLOCK, sample_rate, half_ampl_freq, m);
}

nrf_fir_filter *nrf_fir_filter_new(int sample_rate, int half_ampl_freq, int length) {
    if (length < 1) {
        fprintf(stderr, "NRF FIR fatal error: filter length %d is not >= 1\n", length);
        exit(EXIT_FAILURE);
    }
    nrf_fir_filter *filter = (nrf_fir_filter *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_fir_filter));
    filter->length = length;
    filter->coefficients = nrf_fir_get_low_pass_coefficients(sample_rate, half_ampl_freq, length);
    filter->offset = length - 1;
    filter->center = length / 2;
    filter->samples_length = filter->offset;
    filter->samples = (double *)nrf_private_calloc(BLOCK, (size_t)filter->offset, sizeof(double));
    return filter;
}

void nrf_fir_filter_load(nrf_fir_filter *filter, double *samples, int length) {
    assert(length >= 0);
    const int offset = filter->offset;
    const int new_length = length + offset;
    const double *tail = filter->samples + filter->samples_length - offset;
    if (new_length == filter->samples_length) {
        memmove(filter->samples, tail, sizeof(double) * (size_t)offset); /* regions overlap when length < offset */
    } else {
        double *next = (double *)nrf_private_malloc(BLOCK, sizeof(double) * (size_t)new_length);
        memcpy(next, tail, sizeof(double) * (size_t)offset);
        free(filter->samples);
        filter->samples = next;
        filter->samples_length = new_length;
    }
    memcpy(filter->samples + offset, samples, sizeof(double) * (size_t)length);
}

double nrf_fir_filter_get(nrf_fir_filter *filter, int index) {
    double v = 0;
    for (int i = 0; i < filter->length; i++) v += filter->coefficients[i] * filter->samples[index + i];
    return v;
}

void nrf_fir_filter_free(nrf_fir_filter *filter) {
    if (filter == NULL) return;
    free(filter->coefficients);
    free(filter->samples);
    free(filter);
}

/* ---- IQ filter (GPU) ----------------------------------------------------------- */

nrf_iq_filter *nrf_iq_filter_new(int sample_rate, int half_ampl_freq, int kernel_length) {
    if (kernel_length < 1 || kernel_length > FSEA_FIR_MAX_TAPS) {
        fprintf(stderr, "NRF IQ filter fatal error: kernel length %d is outside [1, %d]\n", kernel_length, FSEA_FIR_MAX_TAPS);
        exit(EXIT_FAILURE);
    }
    nrf_iq_filter *f = (nrf_iq_filter *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_iq_filter));
    nrf_block_init(&f->block, NRF_BLOCK_GENERIC, (nrf_block_process_fn)nrf_iq_filter_process,
                   (nrf_block_result_fn)nrf_iq_filter_get_buffer);
    f->length = kernel_length;
    double *taps = nrf_private_lowpass_taps(BLOCK, sample_rate, half_ampl_freq, kernel_length);
    fsea_fir *fir = NULL;
    const int rc = fsea_fir_create(&fir, taps, kernel_length, nrf_private_device());
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_fir_create", rc);
    free(taps);
    f->backend = fir;
    pthread_mutex_init(&f->mutex, NULL);
    return f;
}

void nrf_iq_filter_process(nrf_iq_filter *filter, nut_buffer *buffer) {
    assert(buffer->channels == 2);
    const int length = buffer->length;
    pthread_mutex_lock(&filter->mutex);
    if (length > filter->output_capacity) {
        free(filter->output);
        filter->output = (float *)nrf_private_malloc(BLOCK, sizeof(float) * 2 * (size_t)length);
        filter->output_capacity = length;
    }
    int rc = FSEA_OK;
    if (buffer->type == NUT_BUFFER_U8) {
        /* u8 / 256 with no flip: nrf_device_get_samples_buffer's bytes are offset binary already */
        rc = fsea_fir_u8_host((fsea_fir *)filter->backend, buffer->data.u8, (size_t)length, 0, filter->output);
    } else {
        rc = fsea_fir_f64_host((fsea_fir *)filter->backend, buffer->data.f64, (size_t)length, filter->output);
    }
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "nrf_iq_filter_process", rc);
    filter->samples_length = length;
    pthread_mutex_unlock(&filter->mutex);
}

nut_buffer *nrf_iq_filter_get_buffer(nrf_iq_filter *f) {
    pthread_mutex_lock(&f->mutex);
    const int length = f->samples_length;
    nut_buffer *result = nut_private_new_f64_unfilled(length, 2);
    nrf_private_widen(result->data.f64, f->output, 2 * length);
    pthread_mutex_unlock(&f->mutex);
    return result;
}

void nrf_iq_filter_free(nrf_iq_filter *filter) {
    if (filter == NULL) return;
    const int rc = fsea_fir_destroy((fsea_fir *)filter->backend);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_fir_destroy", rc);
    pthread_mutex_destroy(&filter->mutex);
    free(filter->output);
    free(filter);
}
