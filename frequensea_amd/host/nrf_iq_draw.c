/*
 * nrf_iq_draw.c -- frequensea's IQ drawing functions and signal detector (include/nrf.h).
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:359-421, 499-553, 876-903.
 *   nrf_buffer_to_iq_points, nrf_device_get_iq_buffer   the per-pair histogram on the GPU (fsea_iq_points_host)
 *   nrf_buffer_to_iq_lines, nrf_device_get_iq_lines     the Bresenham rasteriser on the GPU (fsea_iq_lines_host); the
 *                       number of points (the clamped percentage, in float) is decided here, as in the reference
 *   nrf_buffer_add_position_channel, nrf_signal_detector_*   host arithmetic in double, the reference's loops
 * One draw object per process, created on first use on the device NRF_FFT_DEVICE names (as nrf_iq_filter_new) and
 * guarded by a mutex.
 * Differences: a size_multiplier outside [1, FSEA_IQ_MAX_MULTIPLIER] prints and exits; an incomplete last pair is
 * ignored (the reference reads one element past the buffer); nrf_device_get_iq_* copy the block under data_mutex and
 * release it before the GPU draws.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "IQ draw"

static pthread_mutex_t draw_mutex = PTHREAD_MUTEX_INITIALIZER;
static fsea_iq_draw *draw_backend = NULL; /* created on first use, never freed (one per process) */

void nrf_private_check_iq_multiplier(int size_multiplier) {
    if (size_multiplier < 1 || size_multiplier > FSEA_IQ_MAX_MULTIPLIER) {
        fprintf(stderr, "NRF IQ draw fatal error: size_multiplier %d is outside [1, %d]\n", size_multiplier,
                FSEA_IQ_MAX_MULTIPLIER);
        exit(EXIT_FAILURE);
    }
}

/* the caller holds draw_mutex */
static fsea_iq_draw *backend(void) {
    if (draw_backend == NULL) {
        const int rc = fsea_iq_draw_create(&draw_backend, nrf_private_device());
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_iq_draw_create", rc);
    }
    return draw_backend;
}

static int elements(const nut_buffer *buffer) {
    const int size = buffer->length * buffer->channels;
    return size > 0 ? size : 0;
}

static int iq_type(const nut_buffer *buffer) { return buffer->type == NUT_BUFFER_U8 ? FSEA_IQ_U8 : FSEA_IQ_F64; }

static void draw_points(const void *iq, int type, int n_pairs, nut_buffer *image) {
    pthread_mutex_lock(&draw_mutex);
    const int rc = fsea_iq_points_host(backend(), iq, type, 0, (size_t)n_pairs, image->data.u8);
    pthread_mutex_unlock(&draw_mutex);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_iq_points_host", rc);
}

static void draw_lines(const void *iq, int type, int n_points, int size_multiplier, nut_buffer *image) {
    pthread_mutex_lock(&draw_mutex);
    const int rc = fsea_iq_lines_host(backend(), iq, type, 0, (size_t)n_points, size_multiplier, image->data.u8);
    pthread_mutex_unlock(&draw_mutex);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_iq_lines_host", rc);
}

/* The points the reference's loop `for (i = 0; i < max; i += 2)` visits, max = (int)((float)size * clamped percentage),
 * without an incomplete last pair.  x86-64 turns a NaN or a product of 2^31 or more into INT_MIN: no point. */
int nrf_private_iq_line_points(int size, float line_percentage) {
    const float p = line_percentage < 0 ? 0 : line_percentage > 1 ? 1 : line_percentage; /* _nrf_clampf */
    const float product = (float)size * p;
    if (!(product < 2147483648.0f)) return 0;
    const int max = (int)product;
    const int points = max > 0 ? (max + 1) / 2 : 0;
    return points < size / 2 ? points : size / 2;
}

static nut_buffer *new_image(int side) { return nut_buffer_new_u8(side * side, 1, NULL); }

nut_buffer *nrf_buffer_to_iq_points(nut_buffer *buffer) {
    nut_buffer *image = new_image(NRF_IQ_RESOLUTION);
    draw_points(nrf_private_payload(buffer), iq_type(buffer), elements(buffer) / 2, image);
    return image;
}

nut_buffer *nrf_buffer_to_iq_lines(nut_buffer *buffer, int size_multiplier, float line_percentage) {
    nrf_private_check_iq_multiplier(size_multiplier);
    nut_buffer *image = new_image(NRF_IQ_RESOLUTION * size_multiplier);
    draw_lines(nrf_private_payload(buffer), iq_type(buffer), nrf_private_iq_line_points(elements(buffer), line_percentage),
               size_multiplier, image);
    return image;
}

/* a copy of the device's current block, taken under its lock */
static uint8_t *block_copy(nrf_device *device) {
    uint8_t *copy = (uint8_t *)nrf_private_malloc(BLOCK, NRF_BUFFER_SIZE_BYTES);
    pthread_mutex_lock(&device->data_mutex);
    memcpy(copy, device->samples, NRF_BUFFER_SIZE_BYTES);
    pthread_mutex_unlock(&device->data_mutex);
    return copy;
}

nut_buffer *nrf_device_get_iq_buffer(nrf_device *device) {
    uint8_t *block = block_copy(device);
    nut_buffer *image = new_image(NRF_IQ_RESOLUTION);
    draw_points(block, FSEA_IQ_U8, NRF_BUFFER_SIZE_BYTES / 2, image);
    free(block);
    return image;
}

nut_buffer *nrf_device_get_iq_lines(nrf_device *device, int size_multiplier, float line_percentage) {
    nrf_private_check_iq_multiplier(size_multiplier);
    uint8_t *block = block_copy(device);
    nut_buffer *image = new_image(NRF_IQ_RESOLUTION * size_multiplier);
    draw_lines(block, FSEA_IQ_U8, nrf_private_iq_line_points(NRF_BUFFER_SIZE_BYTES, line_percentage), size_multiplier, image);
    free(block);
    return image;
}

nut_buffer *nrf_buffer_add_position_channel(nut_buffer *buffer) {
    nut_buffer *result = buffer->type == NUT_BUFFER_U8 ? nut_buffer_new_u8(buffer->length, buffer->channels + 1, NULL)
                                                       : nut_buffer_new_f64(buffer->length, buffer->channels + 1, NULL);
    const int size = buffer->length * buffer->channels;
    int k = 0;
    for (int i = 0; i < size; i += buffer->channels) {
        for (int j = 0; j < buffer->channels; j++) nut_buffer_set_f64(result, k++, nut_buffer_get_f64(buffer, i + j));
        nut_buffer_set_f64(result, k++, i / (double)size);
    }
    return result;
}

/* ---- Signal detector (host, double) -------------------------------------------- */

nrf_signal_detector *nrf_signal_detector_new() {
    return (nrf_signal_detector *)nrf_private_calloc("signal detector", 1, sizeof(nrf_signal_detector));
}

void nrf_signal_detector_process(nrf_signal_detector *detector, nut_buffer *buffer) {
    const int size = buffer->length * buffer->channels;
    double total = 0;
    for (int i = 0; i < size; i += 2) total += nut_buffer_get_f64(buffer, i);
    const double mean = total / (double)size * 2;
    double diffs_total = 0;
    for (int i = 0; i < size; i++) {
        const double diff = nut_buffer_get_f64(buffer, i) - mean;
        diffs_total += diff * diff;
    }
    detector->mean = mean;
    detector->standard_deviation = sqrt(diffs_total / mean);
}

void nrf_signal_detector_free(nrf_signal_detector *detector) { free(detector); }
