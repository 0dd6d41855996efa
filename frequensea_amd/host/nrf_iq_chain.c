/*
 * nrf_iq_chain.c -- the IQ chain block (include/nrf.h, an addition beside the reference's prototypes): what the
 * reference's IQ scenes do per block with nrf_freq_shifter, nrf_iq_filter and nrf_buffer_to_iq_points / _lines
 * (lua/dvbt.lua:46-51, lua/iq-tex-filtered.lua:44-47), with the samples staying on the GPU from the 8-bit upload to the
 * image (fsea_chain_*, include/fsea.h).
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:843-866 (the shifter: the offset-binary value
 * is rotated, 0.5 added, into a buffer of twice the input's pairs whose back half stays 0.0), 735-775 (the filter follows
 * buffer->length), 519-553 (the images).  The U8 path does all of it on the device; the F64 path rotates here in double
 * and stages the block through the host.  The phase is closed-form, M * freq_offset / sample_rate cycles after M samples,
 * where the reference steps a (cos, sin) pair.
 * As nrf_iq_filter.c: a kernel length outside [1, FSEA_FIR_MAX_TAPS] prints and exits, a mutex serialises the calls.
 */
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "IQ chain"

static const double TWO_PI = 6.28318530717958647692;

nrf_iq_chain *nrf_iq_chain_new(int sample_rate, int half_ampl_freq, int kernel_length) {
    if (kernel_length < 1 || kernel_length > FSEA_FIR_MAX_TAPS) {
        fprintf(stderr, "NRF IQ chain fatal error: kernel length %d is outside [1, %d]\n", kernel_length, FSEA_FIR_MAX_TAPS);
        exit(EXIT_FAILURE);
    }
    nrf_iq_chain *c = (nrf_iq_chain *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_iq_chain));
    nrf_block_init(&c->block, NRF_BLOCK_GENERIC, (nrf_block_process_fn)nrf_iq_chain_process,
                   (nrf_block_result_fn)nrf_iq_chain_get_buffer);
    c->sample_rate = sample_rate;
    c->length = kernel_length;
    c->samples_length = -1;
    double *taps = nrf_private_lowpass_taps(BLOCK, sample_rate, half_ampl_freq, kernel_length);
    fsea_chain *backend = NULL;
    const int rc = fsea_chain_create(&backend, taps, kernel_length, nrf_private_device());
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_chain_create", rc);
    free(taps);
    c->backend = backend;
    pthread_mutex_init(&c->mutex, NULL);
    return c;
}

void nrf_iq_chain_set_shifter(nrf_iq_chain *chain, int freq_offset) {
    pthread_mutex_lock(&chain->mutex);
    chain->shifting = 1;
    chain->freq_offset = freq_offset;
    chain->consumed = 0;
    pthread_mutex_unlock(&chain->mutex);
}

/* The phase, in [0, 1) cycles, of stream position `position` (< 2^53: exact as a double): cycles_per_sample * position as
 * the exact sum of the rounded product and its fma residual, the product reduced modulo 1 before the residual is added --
 * the two-term reduction of the U8 path's kernel (fsea_fir_stage.h: rot_base) with phase0 = 0, so both inputs of the block
 * are rotated by the same phase however long the stream.  One rounded product alone is off by 1e-5 cycles at 2^40. */
static double phase_cycles(double cycles_per_sample, unsigned long long position) {
    const double k = (double)position;
    const double hi = cycles_per_sample * k;
    const double lo = fma(cycles_per_sample, k, -hi);
    double turns = (hi - floor(hi)) + lo;
    turns -= floor(turns);
    return turns;
}

/* nrf_freq_shifter_process on an F64 buffer: 2 * length pairs, the first `length` rotated + 0.5, the rest 0.0 */
static double *shifted_f64(const nrf_iq_chain *chain, const nut_buffer *buffer, double cycles_per_sample) {
    const int length = buffer->length;
    double *out = (double *)nrf_private_calloc(BLOCK, (size_t)(length > 0 ? length : 1) * 4, sizeof(double));
    for (int k = 0; k < length; k++) {
        const double turns = phase_cycles(cycles_per_sample, chain->consumed + (unsigned long long)k);
        const double c = cos(TWO_PI * turns), s = sin(TWO_PI * turns);
        const double vi = buffer->data.f64[2 * k], vq = buffer->data.f64[2 * k + 1];
        out[2 * k] = vi * c - vq * s + 0.5;
        out[2 * k + 1] = vi * s + vq * c + 0.5;
    }
    return out;
}

void nrf_iq_chain_process(nrf_iq_chain *chain, nut_buffer *buffer) {
    assert(buffer->channels == 2);
    const int length = buffer->length;
    pthread_mutex_lock(&chain->mutex);
    fsea_chain *backend = (fsea_chain *)chain->backend;
    const double cycles_per_sample = (double)chain->freq_offset / (double)chain->sample_rate;
    const int out_length = chain->shifting ? 2 * length : length;
    int rc = FSEA_OK;
    if (buffer->type == NUT_BUFFER_U8) {
        /* u8 / 256 with no flip: nrf_device_get_samples_buffer's bytes are offset binary already */
        fsea_chain_stage stage;
        memset(&stage, 0, sizeof(stage));
        stage.shift = chain->shifting;
        stage.cycles_per_sample = cycles_per_sample;
        stage.sample_offset = chain->consumed;
        stage.n_zero = chain->shifting ? (size_t)length : 0;
        rc = fsea_chain_run_host(backend, buffer->data.u8, (size_t)length, &stage, NULL);
    } else if (chain->shifting) {
        double *rotated = shifted_f64(chain, buffer, cycles_per_sample);
        rc = fsea_chain_run_f64_host(backend, rotated, (size_t)out_length, NULL);
        free(rotated);
    } else {
        rc = fsea_chain_run_f64_host(backend, buffer->data.f64, (size_t)length, NULL);
    }
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "nrf_iq_chain_process", rc);
    if (chain->shifting) chain->consumed += (unsigned long long)length;
    chain->samples_length = out_length;
    pthread_mutex_unlock(&chain->mutex);
}

/* one output of the resident block; the caller holds the mutex */
static void fetch(nrf_iq_chain *chain, const fsea_chain_outputs *outputs) {
    const int rc = fsea_chain_fetch_host((fsea_chain *)chain->backend, outputs);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_chain_fetch_host", rc);
}

nut_buffer *nrf_iq_chain_get_iq_points(nrf_iq_chain *chain) {
    pthread_mutex_lock(&chain->mutex);
    nut_buffer *image = NULL;
    if (chain->samples_length >= 0) {
        image = nut_buffer_new_u8(NRF_IQ_RESOLUTION * NRF_IQ_RESOLUTION, 1, NULL);
        fsea_chain_outputs outputs;
        memset(&outputs, 0, sizeof(outputs));
        outputs.points = image->data.u8;
        fetch(chain, &outputs);
    }
    pthread_mutex_unlock(&chain->mutex);
    return image;
}

nut_buffer *nrf_iq_chain_get_iq_lines(nrf_iq_chain *chain, int size_multiplier, float line_percentage) {
    nrf_private_check_iq_multiplier(size_multiplier);
    pthread_mutex_lock(&chain->mutex);
    nut_buffer *image = NULL;
    if (chain->samples_length >= 0) {
        const int side = NRF_IQ_RESOLUTION * size_multiplier;
        image = nut_buffer_new_u8(side * side, 1, NULL);
        fsea_chain_outputs outputs;
        memset(&outputs, 0, sizeof(outputs));
        outputs.lines = image->data.u8;
        outputs.size_multiplier = size_multiplier;
        /* as nrf_buffer_to_iq_lines on the F64 buffer of get_buffer: 2 * samples_length elements */
        outputs.n_line_points = (size_t)nrf_private_iq_line_points(2 * chain->samples_length, line_percentage);
        fetch(chain, &outputs);
    }
    pthread_mutex_unlock(&chain->mutex);
    return image;
}

nut_buffer *nrf_iq_chain_get_buffer(nrf_iq_chain *chain) {
    pthread_mutex_lock(&chain->mutex);
    nut_buffer *result = NULL;
    if (chain->samples_length >= 0) {
        const int length = chain->samples_length;
        result = nut_private_new_f64_unfilled(length, 2);
        float *pairs = (float *)nrf_private_malloc(BLOCK, sizeof(float) * 2 * (size_t)length);
        fsea_chain_outputs outputs;
        memset(&outputs, 0, sizeof(outputs));
        outputs.pairs = pairs;
        fetch(chain, &outputs);
        nrf_private_widen(result->data.f64, pairs, 2 * length);
        free(pairs);
    }
    pthread_mutex_unlock(&chain->mutex);
    return result;
}

void nrf_iq_chain_free(nrf_iq_chain *chain) {
    if (chain == NULL) return;
    const int rc = fsea_chain_destroy((fsea_chain *)chain->backend);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_chain_destroy", rc);
    pthread_mutex_destroy(&chain->mutex);
    free(chain);
}
