/*
 * nrf_persistence.c -- the persistence-spectrum block (include/nrf.h, an addition beside the reference's prototypes): every
 * frame of a block through a FSEA_MODE_DB5_U8_DCFIX plan on the device and from there into a fsea_persist object
 * (include/fsea.h), whose picture get_buffer returns: 256 levels x fft_size bins, how often each bin was at each level.
 *
 * The reference has no counterpart; the rows are those of its c/fft-batch.c pixel mapping (the DB5 mode), the picture is
 * what ngl_texture_update(texture, buffer, fft_size, 256) takes.  The block goes up once per process call and no row comes
 * back: the plan writes its rows into device memory of the block and the object counts them there.
 * As nrf_pfb_fft.c: a parameter out of range prints and exits, a mutex serialises the calls.
 */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "PERSISTENCE"

nrf_persistence *nrf_persistence_new(int fft_size, int hop, int map) {
    if (fft_size < 1 || fft_size > FSEA_PERSIST_MAX_WIDTH) {
        fprintf(stderr, "NRF PERSISTENCE fatal error: fft size %d is outside [1, %d]\n", fft_size, FSEA_PERSIST_MAX_WIDTH);
        exit(EXIT_FAILURE);
    }
    if (hop < 1) {
        fprintf(stderr, "NRF PERSISTENCE fatal error: hop %d is not positive\n", hop);
        exit(EXIT_FAILURE);
    }
    if (map != FSEA_PERSIST_MAP_SATURATE && map != FSEA_PERSIST_MAP_LINEAR && map != FSEA_PERSIST_MAP_LOG) {
        fprintf(stderr, "NRF PERSISTENCE fatal error: map %d is not one of FSEA_PERSIST_MAP_*\n", map);
        exit(EXIT_FAILURE);
    }
    nrf_persistence *p = (nrf_persistence *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_persistence));
    nrf_block_init(&p->block, NRF_BLOCK_GENERIC, (nrf_block_process_fn)nrf_persistence_process,
                   (nrf_block_result_fn)nrf_persistence_get_buffer);
    p->fft_size = fft_size;
    p->hop = hop;
    p->map = map;
    p->decay_numerator = p->decay_denominator = 1;
    p->device = nrf_private_device();
    fsea_plan *plan = NULL;
    int rc = fsea_plan_create(&plan, fft_size, hop, FSEA_MODE_DB5_U8_DCFIX, p->device);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_plan_create", rc);
    p->plan = plan;
    fsea_persist *persist = NULL;
    rc = fsea_persist_create(&persist, fft_size, p->device);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_persist_create", rc);
    p->backend = persist;
    pthread_mutex_init(&p->mutex, NULL);
    return p;
}

void nrf_persistence_set_window(nrf_persistence *p, const char *name) {
    nrf_private_check_window_name(BLOCK, "nrf_persistence_set_window", name);
    pthread_mutex_lock(&p->mutex);
    nrf_private_set_window(BLOCK, NULL, (fsea_plan *)p->plan, p->fft_size, name);
    pthread_mutex_unlock(&p->mutex);
}

void nrf_persistence_set_decay(nrf_persistence *p, unsigned numerator, unsigned denominator) {
    if (denominator < 1 || numerator > denominator) {
        fprintf(stderr, "NRF PERSISTENCE fatal error: decay %u / %u needs 1 <= denominator and numerator <= denominator\n",
                numerator, denominator);
        exit(EXIT_FAILURE);
    }
    pthread_mutex_lock(&p->mutex);
    p->decay_numerator = numerator;
    p->decay_denominator = denominator;
    pthread_mutex_unlock(&p->mutex);
}

void nrf_persistence_process(nrf_persistence *p, nut_buffer *buffer) {
    assert(buffer->channels == 2);
    nrf_private_need_u8(BLOCK, buffer);
    const size_t n = (size_t)p->fft_size;
    pthread_mutex_lock(&p->mutex);
    fsea_persist *persist = (fsea_persist *)p->backend;
    int rc = fsea_persist_decay(persist, p->decay_numerator, p->decay_denominator, NULL);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_persist_decay", rc);
    const size_t frames = nrf_private_rows_on_device(BLOCK, p->device, (fsea_plan *)p->plan, n, (size_t)p->hop, buffer, &p->d_iq,
                                                     &p->iq_cap, &p->d_rows, &p->rows_cap);
    if (frames) {
        rc = fsea_persist_add_device(persist, p->d_rows, FSEA_PERSIST_U8, frames, n, NULL);
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_persist_add_device", rc);
    }
    pthread_mutex_unlock(&p->mutex);
}

nut_buffer *nrf_persistence_get_buffer(nrf_persistence *p) {
    pthread_mutex_lock(&p->mutex);
    nut_buffer *result = nut_buffer_new_u8(FSEA_PERSIST_LEVELS * p->fft_size, 1, NULL);
    const int rc = fsea_persist_image_host((fsea_persist *)p->backend, p->map, 0, result->data.u8);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_persist_image_host", rc);
    pthread_mutex_unlock(&p->mutex);
    return result;
}

void nrf_persistence_free(nrf_persistence *p) {
    if (p == NULL) return;
    int rc = fsea_persist_destroy((fsea_persist *)p->backend);   /* waits for the device */
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_persist_destroy", rc);
    rc = fsea_plan_destroy((fsea_plan *)p->plan);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_plan_destroy", rc);
    if (p->d_iq != NULL) fsea_device_free(p->device, p->d_iq);
    if (p->d_rows != NULL) fsea_device_free(p->device, p->d_rows);
    pthread_mutex_destroy(&p->mutex);
    free(p);
}
