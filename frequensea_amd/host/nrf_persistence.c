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
#include <string.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "PERSISTENCE"

static void grow(int device, void **d_ptr, size_t *cap, size_t need) {
    if (*cap >= need) return;
    int rc = *d_ptr != NULL ? fsea_device_free(device, *d_ptr) : FSEA_OK;
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_device_free", rc);
    *d_ptr = NULL;
    *cap = 0;
    rc = fsea_device_alloc(device, need, d_ptr);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_device_alloc", rc);
    *cap = need;
}

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
    static const char *names[] = {"rect", "hann", "hamming", "blackman", "blackmanharris", "flattop"};   /* FSEA_WINDOW_* */
    int kind = -1;
    if (name == NULL || name[0] == '\0' || strcmp(name, "none") == 0) kind = 0;
    for (int k = 0; k < 6 && kind < 0; k++) {
        if (strcmp(name, names[k]) == 0) kind = k;
    }
    if (kind < 0) {
        fprintf(stderr, "NRF PERSISTENCE fatal error: nrf_persistence_set_window: \"%s\" is not one of hann, hamming, blackman, "
                        "blackmanharris, flattop, rect\n", name);
        exit(EXIT_FAILURE);
    }
    pthread_mutex_lock(&p->mutex);
    int rc;
    if (kind == 0) {
        rc = fsea_plan_set_window((fsea_plan *)p->plan, NULL);
    } else {
        float *w = (float *)nrf_private_malloc(BLOCK, sizeof(float) * (size_t)p->fft_size);
        rc = fsea_window_fill(kind, p->fft_size, w);
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_window_fill", rc);
        rc = fsea_plan_set_window((fsea_plan *)p->plan, w);
        free(w);
    }
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_plan_set_window", rc);
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
    if (buffer->type != NUT_BUFFER_U8) {
        fprintf(stderr, "NRF PERSISTENCE fatal error: the block takes 8-bit samples, not an F64 buffer\n");
        exit(EXIT_FAILURE);
    }
    const size_t length = (size_t)buffer->length, n = (size_t)p->fft_size;
    pthread_mutex_lock(&p->mutex);
    fsea_persist *persist = (fsea_persist *)p->backend;
    int rc = fsea_persist_decay(persist, p->decay_numerator, p->decay_denominator, NULL);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_persist_decay", rc);
    if (length >= n) {
        const size_t frames = (length - n) / (size_t)p->hop + 1;
        grow(p->device, &p->d_iq, &p->iq_cap, 2 * length);
        grow(p->device, &p->d_rows, &p->rows_cap, frames * n);
        /* everything on the null stream, in order; u8 / 256 with no flip: nrf_device_get_samples_buffer's bytes are offset
         * binary already */
        rc = fsea_copy_to_device(p->device, p->d_iq, buffer->data.u8, 2 * length);
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_copy_to_device", rc);
        rc = fsea_exec_u8_device((fsea_plan *)p->plan, p->d_iq, frames, 0, p->d_rows, NULL);
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_exec_u8_device", rc);
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
