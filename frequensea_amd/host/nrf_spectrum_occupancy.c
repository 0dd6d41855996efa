/*
 * nrf_spectrum_occupancy.c -- the spectrum-occupancy block (include/nrf.h, an addition beside the reference's prototypes):
 * every frame of a block through a FSEA_MODE_DB5_U8_DCFIX plan on the device and from there into a fsea_cfar object
 * (include/fsea.h), the CFAR detector across frequency.  get_buffer returns the duty cycle of every bin, hits[k] / rows, over
 * all the blocks processed; get_mask_buffer the detections of the last block, one byte per frame and bin.
 *
 * The reference has no counterpart: its only spectrum-side detector is the 100-row gate of c/fft-batch-broad.c, which keeps
 * or drops a whole centre frequency.  The block goes up once per process call and nothing comes back: the plan writes its
 * rows into device memory of the block, the object decides them there and leaves the mask on the device until it is asked
 * for.  As nrf_persistence.c: a parameter out of range prints and exits, a mutex serialises the calls.
 */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "SPECTRUM OCCUPANCY"

nrf_spectrum_occupancy *nrf_spectrum_occupancy_new(int fft_size, int hop, int guard, int train, int offset, int method) {
    if (fft_size < 1 || fft_size > FSEA_CFAR_MAX_WIDTH) {
        fprintf(stderr, "NRF SPECTRUM OCCUPANCY fatal error: fft size %d is outside [1, %d]\n", fft_size, FSEA_CFAR_MAX_WIDTH);
        exit(EXIT_FAILURE);
    }
    if (hop < 1) {
        fprintf(stderr, "NRF SPECTRUM OCCUPANCY fatal error: hop %d is not positive\n", hop);
        exit(EXIT_FAILURE);
    }
    if (guard < 0 || guard > FSEA_CFAR_MAX_GUARD) {
        fprintf(stderr, "NRF SPECTRUM OCCUPANCY fatal error: guard %d is outside [0, %d]\n", guard, FSEA_CFAR_MAX_GUARD);
        exit(EXIT_FAILURE);
    }
    if (train < 1 || train > FSEA_CFAR_MAX_TRAIN) {
        fprintf(stderr, "NRF SPECTRUM OCCUPANCY fatal error: train %d is outside [1, %d]\n", train, FSEA_CFAR_MAX_TRAIN);
        exit(EXIT_FAILURE);
    }
    if (offset < -FSEA_CFAR_MAX_OFFSET || offset > FSEA_CFAR_MAX_OFFSET) {
        fprintf(stderr, "NRF SPECTRUM OCCUPANCY fatal error: offset %d is outside [-%d, %d]\n", offset, FSEA_CFAR_MAX_OFFSET,
                FSEA_CFAR_MAX_OFFSET);
        exit(EXIT_FAILURE);
    }
    if (method != FSEA_CFAR_CA && method != FSEA_CFAR_GO && method != FSEA_CFAR_SO) {
        fprintf(stderr, "NRF SPECTRUM OCCUPANCY fatal error: method %d is not one of FSEA_CFAR_CA, FSEA_CFAR_GO, FSEA_CFAR_SO\n", method);
        exit(EXIT_FAILURE);
    }
    nrf_spectrum_occupancy *p = (nrf_spectrum_occupancy *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_spectrum_occupancy));
    nrf_block_init(&p->block, NRF_BLOCK_GENERIC, (nrf_block_process_fn)nrf_spectrum_occupancy_process,
                   (nrf_block_result_fn)nrf_spectrum_occupancy_get_buffer);
    p->fft_size = fft_size;
    p->hop = hop;
    p->device = nrf_private_device();
    fsea_plan *plan = NULL;
    int rc = fsea_plan_create(&plan, fft_size, hop, FSEA_MODE_DB5_U8_DCFIX, p->device);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_plan_create", rc);
    p->plan = plan;
    fsea_cfar *cfar = NULL;
    rc = fsea_cfar_create(&cfar, fft_size, p->device);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_cfar_create", rc);
    p->backend = cfar;
    rc = fsea_cfar_set(cfar, guard, train, offset, method);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_cfar_set", rc);
    pthread_mutex_init(&p->mutex, NULL);
    return p;
}

void nrf_spectrum_occupancy_set_window(nrf_spectrum_occupancy *p, const char *name) {
    nrf_private_check_window_name(BLOCK, "nrf_spectrum_occupancy_set_window", name);
    pthread_mutex_lock(&p->mutex);
    nrf_private_set_window(BLOCK, NULL, (fsea_plan *)p->plan, p->fft_size, name);
    pthread_mutex_unlock(&p->mutex);
}

void nrf_spectrum_occupancy_process(nrf_spectrum_occupancy *p, nut_buffer *buffer) {
    assert(buffer->channels == 2);
    nrf_private_need_u8(BLOCK, buffer);
    const size_t n = (size_t)p->fft_size;
    pthread_mutex_lock(&p->mutex);
    p->mask_rows = 0;
    const size_t frames = nrf_private_rows_on_device(BLOCK, p->device, (fsea_plan *)p->plan, n, (size_t)p->hop, buffer, &p->d_iq,
                                                     &p->iq_cap, &p->d_rows, &p->rows_cap);
    if (frames) {
        nrf_private_grow(BLOCK, p->device, &p->d_mask, &p->mask_cap, frames * n);
        const int rc = fsea_cfar_add_device((fsea_cfar *)p->backend, p->d_rows, FSEA_CFAR_U8, frames, n, (uint8_t *)p->d_mask, NULL, NULL);
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_cfar_add_device", rc);
        p->mask_rows = frames;
    }
    pthread_mutex_unlock(&p->mutex);
}

nut_buffer *nrf_spectrum_occupancy_get_buffer(nrf_spectrum_occupancy *p) {
    pthread_mutex_lock(&p->mutex);
    const size_t n = (size_t)p->fft_size;
    nut_buffer *result = nut_buffer_new_f64(p->fft_size, 1, NULL);
    uint32_t *hits = (uint32_t *)nrf_private_malloc(BLOCK, sizeof(uint32_t) * n);
    const int rc = fsea_cfar_hits_host((fsea_cfar *)p->backend, hits);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_cfar_hits_host", rc);
    const uint64_t rows = fsea_cfar_rows((fsea_cfar *)p->backend);
    for (size_t k = 0; k < n; k++) result->data.f64[k] = rows ? (double)hits[k] / (double)rows : 0.0;
    free(hits);
    pthread_mutex_unlock(&p->mutex);
    return result;
}

nut_buffer *nrf_spectrum_occupancy_get_mask_buffer(nrf_spectrum_occupancy *p) {
    pthread_mutex_lock(&p->mutex);
    const size_t bytes = p->mask_rows * (size_t)p->fft_size;
    nut_buffer *result = nut_buffer_new_u8((int)bytes, 1, NULL);
    if (bytes) {
        const int rc = fsea_copy_to_host(p->device, result->data.u8, p->d_mask, bytes);   /* waits for the null stream's work */
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_copy_to_host", rc);
    }
    pthread_mutex_unlock(&p->mutex);
    return result;
}

void nrf_spectrum_occupancy_free(nrf_spectrum_occupancy *p) {
    if (p == NULL) return;
    int rc = fsea_cfar_destroy((fsea_cfar *)p->backend);   /* waits for the device */
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_cfar_destroy", rc);
    rc = fsea_plan_destroy((fsea_plan *)p->plan);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_plan_destroy", rc);
    if (p->d_iq != NULL) fsea_device_free(p->device, p->d_iq);
    if (p->d_rows != NULL) fsea_device_free(p->device, p->d_rows);
    if (p->d_mask != NULL) fsea_device_free(p->device, p->d_mask);
    pthread_mutex_destroy(&p->mutex);
    free(p);
}
