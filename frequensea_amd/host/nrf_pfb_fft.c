/*
 * nrf_pfb_fft.c -- the filter-bank spectrum block (include/nrf.h, an addition beside the reference's prototypes): nrf_fft with
 * a polyphase filter bank in front of the transform (fsea_pfb_*, include/fsea.h), for the scenes that draw nrf_fft's history.
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:594-642 -- MAG rows with the DC bin replaced, bin
 * fft_size / 2 the centre, the history scrolled newest row first.  The bank has no counterpart there: fft_size channels, the
 * prototype of fsea_pfb_prototype, a row every fft_size samples, all rows of a block.
 * As nrf_zoom_fft.c: a parameter out of range prints and exits, a mutex serialises the calls.
 */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "PFB FFT"

nrf_pfb_fft *nrf_pfb_fft_new(int fft_size, int fft_history_size, int branch_taps) {
    if (fft_size < 2 || fft_size > FSEA_PFB_MAX_CHANNELS || fft_size % 2 != 0) {
        fprintf(stderr, "NRF PFB FFT fatal error: fft size %d is odd or outside [2, %d]\n", fft_size, FSEA_PFB_MAX_CHANNELS);
        exit(EXIT_FAILURE);
    }
    if (branch_taps < 1 || branch_taps > FSEA_PFB_MAX_BRANCH_TAPS) {
        fprintf(stderr, "NRF PFB FFT fatal error: branch taps %d is outside [1, %d]\n", branch_taps, FSEA_PFB_MAX_BRANCH_TAPS);
        exit(EXIT_FAILURE);
    }
    if (fft_history_size < 1) {
        fprintf(stderr, "NRF PFB FFT fatal error: history size %d is not positive\n", fft_history_size);
        exit(EXIT_FAILURE);
    }
    nrf_pfb_fft *p = (nrf_pfb_fft *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_pfb_fft));
    nrf_block_init(&p->block, NRF_BLOCK_GENERIC, (nrf_block_process_fn)nrf_pfb_fft_process,
                   (nrf_block_result_fn)nrf_pfb_fft_get_buffer);
    p->fft_size = fft_size;
    p->fft_history_size = fft_history_size;
    p->branch_taps = branch_taps;
    double *taps = (double *)nrf_private_malloc(BLOCK, sizeof(double) * (size_t)fft_size * (size_t)branch_taps);
    int rc = fsea_pfb_prototype(fft_size, branch_taps, taps);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_pfb_prototype", rc);
    fsea_pfb *backend = NULL;
    rc = fsea_pfb_create(&backend, taps, fft_size, branch_taps, 1, FSEA_MODE_MAG_F32, nrf_private_device());
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_pfb_create", rc);
    free(taps);
    p->backend = backend;
    p->history = (double *)nrf_private_calloc(BLOCK, (size_t)fft_size * (size_t)fft_history_size, sizeof(double));
    pthread_mutex_init(&p->mutex, NULL);
    return p;
}

void nrf_pfb_fft_process(nrf_pfb_fft *pfb, nut_buffer *buffer) {
    assert(buffer->channels == 2);
    nrf_private_need_u8(BLOCK, buffer);
    const size_t length = (size_t)buffer->length, n = (size_t)pfb->fft_size, history = (size_t)pfb->fft_history_size;
    pthread_mutex_lock(&pfb->mutex);
    fsea_pfb *backend = (fsea_pfb *)pfb->backend;
    const size_t rows = fsea_pfb_out_frames(backend, length);
    float *fresh = (float *)nrf_private_malloc(BLOCK, sizeof(float) * rows * n);
    /* u8 / 256 with no flip: nrf_device_get_samples_buffer's bytes are offset binary already */
    const int rc = fsea_pfb_run_host(backend, buffer->data.u8, length, 0, fresh, NULL, NULL);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_pfb_run_host", rc);
    /* scroll: the block's rows enter oldest first, so its last row ends as row 0 and the newest `history` rows remain */
    const size_t keep = rows < history ? rows : history;
    memmove(pfb->history + keep * n, pfb->history, sizeof(double) * (history - keep) * n);
    for (size_t r = 0; r < keep; r++) nrf_private_widen(pfb->history + r * n, fresh + (rows - 1 - r) * n, (int)n);
    free(fresh);
    pthread_mutex_unlock(&pfb->mutex);
}

nut_buffer *nrf_pfb_fft_get_buffer(nrf_pfb_fft *pfb) {
    pthread_mutex_lock(&pfb->mutex);
    const int count = pfb->fft_size * pfb->fft_history_size;
    nut_buffer *result = nut_private_new_f64_unfilled(count, 1);
    memcpy(result->data.f64, pfb->history, sizeof(double) * (size_t)count);
    pthread_mutex_unlock(&pfb->mutex);
    return result;
}

void nrf_pfb_fft_free(nrf_pfb_fft *pfb) {
    if (pfb == NULL) return;
    const int rc = fsea_pfb_destroy((fsea_pfb *)pfb->backend);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_pfb_destroy", rc);
    pthread_mutex_destroy(&pfb->mutex);
    free(pfb->history);
    free(pfb);
}
