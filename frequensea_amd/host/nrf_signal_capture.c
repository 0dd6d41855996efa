/*
 * nrf_signal_capture.c -- the signal capture block (include/nrf.h, an addition beside the reference's prototypes): what the
 * reference's signal scene does block by block with nrf_signal_detector, nrf_iq_filter, nut_buffer_append and
 * nrf_buffer_to_iq_lines (lua/signal-detector.lua:89-133), over a whole recording that stays on the GPU from the upload to
 * the image (fsea_capture_*, include/fsea.h).
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:883-898 (the detector: mean of the even
 * elements times 2, the squared differences divided by the mean), lua/signal-detector.lua:92-113 (a block above the
 * threshold starts or continues a burst and is filtered and appended; the first one at or below it ends the burst and is
 * dropped), 114-131 (the burst drawn as a growing line image).  The scene's threshold is 100 and its filter
 * (sample_rate, 200e3, 97); one filter serves the whole scene, its tail carried from one gated block to the next.
 * As nrf_iq_chain.c: a kernel length outside [1, FSEA_FIR_MAX_TAPS] prints and exits, as does a backend failure; a mutex
 * serialises the calls.
 */
#include <assert.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "signal capture"

nrf_signal_capture *nrf_signal_capture_new(int sample_rate, int half_ampl_freq, int kernel_length, double threshold) {
    if (kernel_length < 1 || kernel_length > FSEA_FIR_MAX_TAPS) {
        fprintf(stderr, "NRF signal capture fatal error: kernel length %d is outside [1, %d]\n", kernel_length,
                FSEA_FIR_MAX_TAPS);
        exit(EXIT_FAILURE);
    }
    nrf_signal_capture *c = (nrf_signal_capture *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_signal_capture));
    c->sample_rate = sample_rate;
    c->length = kernel_length;
    c->threshold = threshold;
    double *taps = nrf_private_lowpass_taps(BLOCK, sample_rate, half_ampl_freq, kernel_length);
    fsea_capture *backend = NULL;
    const int rc = fsea_capture_create(&backend, taps, kernel_length, nrf_private_device());
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_capture_create", rc);
    free(taps);
    c->backend = backend;
    pthread_mutex_init(&c->mutex, NULL);
    return c;
}

int nrf_signal_capture_scan(nrf_signal_capture *capture, nut_buffer *recording, int block_length) {
    assert(recording->type == NUT_BUFFER_U8 && recording->channels == 2);
    if (block_length < 1) {
        fprintf(stderr, "NRF signal capture fatal error: block length %d is not >= 1\n", block_length);
        exit(EXIT_FAILURE);
    }
    pthread_mutex_lock(&capture->mutex);
    fsea_capture *backend = (fsea_capture *)capture->backend;
    const size_t n_blocks = (size_t)(recording->length > 0 ? recording->length : 0) / (size_t)block_length;
    if (n_blocks > 0) {
        /* u8 / 256 with no flip: nrf_device_get_samples_buffer's bytes are offset binary already */
        const int rc = fsea_capture_scan_host(backend, recording->data.u8, 2 * (size_t)block_length, n_blocks, 0,
                                              capture->threshold);
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "nrf_signal_capture_scan", rc);
    }
    const int bursts = (int)fsea_capture_n_bursts(backend);
    pthread_mutex_unlock(&capture->mutex);
    return bursts;
}

/* the caller holds the mutex */
static void stats(nrf_signal_capture *capture, int block, double *mean, double *sd) {
    /* a negative index is out of range as a size_t too */
    const int rc = fsea_capture_stats((fsea_capture *)capture->backend, (size_t)block, mean, sd);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_capture_stats", rc);
}

double nrf_signal_capture_get_mean(nrf_signal_capture *capture, int block) {
    double mean, sd;
    pthread_mutex_lock(&capture->mutex);
    stats(capture, block, &mean, &sd);
    pthread_mutex_unlock(&capture->mutex);
    return mean;
}

double nrf_signal_capture_get_standard_deviation(nrf_signal_capture *capture, int block) {
    double mean, sd;
    pthread_mutex_lock(&capture->mutex);
    stats(capture, block, &mean, &sd);
    pthread_mutex_unlock(&capture->mutex);
    return sd;
}

/* the caller holds the mutex; a burst whose elements an int cannot count has no nut_buffer */
static fsea_capture_burst_info burst_info(nrf_signal_capture *capture, int burst) {
    fsea_capture_burst_info info;
    const int rc = fsea_capture_burst((fsea_capture *)capture->backend, (size_t)burst, &info);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_capture_burst", rc);
    if (info.n_pairs > (size_t)INT_MAX / 2) {
        fprintf(stderr, "NRF signal capture fatal error: burst %d has %zu pairs, more than a buffer holds\n", burst, info.n_pairs);
        exit(EXIT_FAILURE);
    }
    return info;
}

nut_buffer *nrf_signal_capture_get_burst(nrf_signal_capture *capture, int burst) {
    pthread_mutex_lock(&capture->mutex);
    const fsea_capture_burst_info info = burst_info(capture, burst);
    const int length = (int)info.n_pairs;
    nut_buffer *result = nut_private_new_f64_unfilled(length, 2);
    float *pairs = (float *)nrf_private_malloc(BLOCK, sizeof(float) * 2 * (size_t)length);
    const int rc = fsea_capture_burst_pairs_host((fsea_capture *)capture->backend, (size_t)burst, pairs);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_capture_burst_pairs_host", rc);
    nrf_private_widen(result->data.f64, pairs, 2 * length);
    free(pairs);
    pthread_mutex_unlock(&capture->mutex);
    return result;
}

nut_buffer *nrf_signal_capture_get_iq_lines(nrf_signal_capture *capture, int burst, int size_multiplier, float line_percentage) {
    nrf_private_check_iq_multiplier(size_multiplier);
    pthread_mutex_lock(&capture->mutex);
    const fsea_capture_burst_info info = burst_info(capture, burst);
    const int side = NRF_IQ_RESOLUTION * size_multiplier;
    nut_buffer *image = nut_buffer_new_u8(side * side, 1, NULL);
    /* as nrf_buffer_to_iq_lines on the F64 buffer of get_burst: 2 * n_pairs elements */
    const size_t points = (size_t)nrf_private_iq_line_points(2 * (int)info.n_pairs, line_percentage);
    const int rc = fsea_capture_burst_lines_host((fsea_capture *)capture->backend, (size_t)burst, size_multiplier, points,
                                                 image->data.u8);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_capture_burst_lines_host", rc);
    pthread_mutex_unlock(&capture->mutex);
    return image;
}

void nrf_signal_capture_free(nrf_signal_capture *capture) {
    if (capture == NULL) return;
    const int rc = fsea_capture_destroy((fsea_capture *)capture->backend);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_capture_destroy", rc);
    pthread_mutex_destroy(&capture->mutex);
    free(capture);
}
