/*
 * nrf_zoom_fft.c -- the zoom spectrum block (include/nrf.h, an addition beside the reference's prototypes): the chain the
 * reference runs inside nrf_decoder -- nrf_freq_shifter -> nrf_downsampler -> nrf_fft -- as one block whose result is a
 * spectrum history of 1 / decimation of the bandwidth (fsea_zoom_*, include/fsea.h).
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:843-866 (the shifter: the offset-binary value is
 * rotated, 0.5 added), nrf_downsampler_process (the low-pass of nrf_fir_get_low_pass_coefficients evaluated at every
 * rate_mul-th sample, t restarted with every block), 594-642 (the FFT's MAG rows with the DC bin replaced, newest row
 * first).  The phase is closed-form, M * freq_offset / sample_rate cycles after M samples, where the reference steps a
 * (cos, sin) pair.
 * As nrf_iq_chain.c: a kernel length or decimation out of range prints and exits, a mutex serialises the calls.
 */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "zoom FFT"

nrf_zoom_fft *nrf_zoom_fft_new(int sample_rate, int freq_offset, int decimation, int half_ampl_freq, int kernel_length,
                               int fft_size, int fft_history_size) {
    if (kernel_length < 1 || kernel_length > FSEA_FIR_MAX_TAPS) {
        fprintf(stderr, "NRF zoom FFT fatal error: kernel length %d is outside [1, %d]\n", kernel_length, FSEA_FIR_MAX_TAPS);
        exit(EXIT_FAILURE);
    }
    if (decimation < 1 || decimation > FSEA_ZOOM_MAX_DECIMATION) {
        fprintf(stderr, "NRF zoom FFT fatal error: decimation %d is outside [1, %d]\n", decimation, FSEA_ZOOM_MAX_DECIMATION);
        exit(EXIT_FAILURE);
    }
    if (fft_history_size < 1) {
        fprintf(stderr, "NRF zoom FFT fatal error: history size %d is not positive\n", fft_history_size);
        exit(EXIT_FAILURE);
    }
    nrf_zoom_fft *z = (nrf_zoom_fft *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_zoom_fft));
    nrf_block_init(&z->block, NRF_BLOCK_GENERIC, (nrf_block_process_fn)nrf_zoom_fft_process,
                   (nrf_block_result_fn)nrf_zoom_fft_get_buffer);
    z->sample_rate = sample_rate;
    z->freq_offset = freq_offset;
    z->decimation = decimation;
    z->fft_size = fft_size;
    z->fft_history_size = fft_history_size;
    double *taps = nrf_private_lowpass_taps(BLOCK, sample_rate, half_ampl_freq, kernel_length);
    fsea_zoom *backend = NULL;
    const int rc = fsea_zoom_create(&backend, taps, kernel_length, decimation, fft_size, fft_size, FSEA_MODE_MAG_F32,
                                    nrf_private_device());
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_zoom_create", rc);
    free(taps);
    z->backend = backend;
    z->history = (double *)nrf_private_calloc(BLOCK, (size_t)fft_size * (size_t)fft_history_size, sizeof(double));
    pthread_mutex_init(&z->mutex, NULL);
    return z;
}

void nrf_zoom_fft_set_freq_offset(nrf_zoom_fft *zoom, int freq_offset) {
    pthread_mutex_lock(&zoom->mutex);
    zoom->freq_offset = freq_offset;
    zoom->consumed = 0;
    const int rc = fsea_zoom_reset((fsea_zoom *)zoom->backend);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_zoom_reset", rc);
    pthread_mutex_unlock(&zoom->mutex);
}

void nrf_zoom_fft_process(nrf_zoom_fft *zoom, nut_buffer *buffer) {
    assert(buffer->channels == 2);
    nrf_private_need_u8(BLOCK, buffer);
    const size_t length = (size_t)buffer->length, n = (size_t)zoom->fft_size, history = (size_t)zoom->fft_history_size;
    pthread_mutex_lock(&zoom->mutex);
    fsea_zoom *backend = (fsea_zoom *)zoom->backend;
    const size_t rows = fsea_zoom_out_rows(backend, length);
    float *fresh = (float *)nrf_private_malloc(BLOCK, sizeof(float) * rows * n);
    /* u8 / 256 with no flip: nrf_device_get_samples_buffer's bytes are offset binary already */
    const int rc = fsea_zoom_run_host(backend, buffer->data.u8, length, 0, (double)zoom->freq_offset / (double)zoom->sample_rate,
                                      0.0, zoom->consumed, fresh, NULL);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_zoom_run_host", rc);
    zoom->consumed += (unsigned long long)length;
    /* scroll: the block's rows enter oldest first, so its last row ends as row 0 and the newest `history` rows remain */
    const size_t keep = rows < history ? rows : history;
    memmove(zoom->history + keep * n, zoom->history, sizeof(double) * (history - keep) * n);
    for (size_t r = 0; r < keep; r++) nrf_private_widen(zoom->history + r * n, fresh + (rows - 1 - r) * n, (int)n);
    free(fresh);
    pthread_mutex_unlock(&zoom->mutex);
}

nut_buffer *nrf_zoom_fft_get_buffer(nrf_zoom_fft *zoom) {
    pthread_mutex_lock(&zoom->mutex);
    const int count = zoom->fft_size * zoom->fft_history_size;
    nut_buffer *result = nut_private_new_f64_unfilled(count, 1);
    memcpy(result->data.f64, zoom->history, sizeof(double) * (size_t)count);
    pthread_mutex_unlock(&zoom->mutex);
    return result;
}

void nrf_zoom_fft_free(nrf_zoom_fft *zoom) {
    if (zoom == NULL) return;
    const int rc = fsea_zoom_destroy((fsea_zoom *)zoom->backend);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_zoom_destroy", rc);
    pthread_mutex_destroy(&zoom->mutex);
    free(zoom->history);
    free(zoom);
}
