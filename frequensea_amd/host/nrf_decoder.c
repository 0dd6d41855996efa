/*
 * nrf_decoder.c -- frequensea's downsampler, RAW and WBFM demodulators and decoder (include/nrf.h).
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:778-811, 904-1094.
 *   nrf_downsampler_*       host arithmetic in double on nrf_fir_filter_*, the reference's loop bit for bit
 *   nrf_raw_demodulator_*,  one 1-channel fsea_demod (include/fsea.h) with offset 0, f64 form: the whole chain on the GPU
 *   nrf_fm_demodulator_*
 *   nrf_decoder_*           one 1-channel fsea_demod, u8 form, offset and phase taken from the decoder's freq_shifter
 * Differences (include/nrf.h): intermediate arrays are not kept, l_i / l_q / deemphasis_val live on the
 * device, the phase comes from an exactly reduced cycle count, and a backend failure prints and exits.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "decoder"

static const double TAU = 6.28318530717958647692;
static const int FM_INTER_RATE = 336000;
static const int FM_MAX_F = 75000;

/* ---- Downsampler (host, double) ------------------------------------------------ */

nrf_downsampler *nrf_downsampler_new(int in_rate, int out_rate, int filter_freq, int kernel_length) {
    nrf_downsampler *d = (nrf_downsampler *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_downsampler));
    d->in_rate = in_rate;
    d->out_rate = out_rate;
    d->filter = nrf_fir_filter_new(in_rate, filter_freq, kernel_length);
    d->rate_mul = in_rate / (double)out_rate;
    d->out_length = 0;
    d->out_samples = NULL;
    return d;
}

void nrf_downsampler_process(nrf_downsampler *d, double *samples, int length) {
    nrf_fir_filter_load(d->filter, samples, length);
    free(d->out_samples);
    d->out_length = (int)floor(length / d->rate_mul);
    d->out_samples = (double *)nrf_private_calloc(BLOCK, (size_t)d->out_length, sizeof(double));
    double t = 0;
    for (int i = 0; i < d->out_length; i++) {
        d->out_samples[i] = nrf_fir_filter_get(d->filter, (int)floor(t));
        t += d->rate_mul;
    }
}

void nrf_downsampler_free(nrf_downsampler *d) {
    if (d == NULL) return;
    nrf_fir_filter_free(d->filter);
    free(d->out_samples);
    free(d);
}

/* ---- the GPU backend ------------------------------------------------------------- */

static fsea_demod *backend_new(int type, int in_rate, int out_rate) {
    fsea_demod *b = NULL;
    const int rc = fsea_demod_create(&b, type, in_rate, out_rate, 1, nrf_private_device());
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_demod_create", rc);
    return b;
}

static void backend_free(void *b) {
    if (b == NULL) return;
    const int rc = fsea_demod_destroy((fsea_demod *)b);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_demod_destroy", rc);
}

/* the demodulator's audio buffer sized for a call on `length` samples (reallocated when the length changes, as upstream) */
static double *audio_buffer(fsea_demod *b, double **audio, int *audio_length, int length) {
    const int n = (int)fsea_demod_out_length(b, (size_t)length);
    if (n != *audio_length || *audio == NULL) {
        free(*audio);
        *audio = (double *)nrf_private_calloc(BLOCK, (size_t)n, sizeof(double));
        *audio_length = n;
    }
    return *audio;
}

/* nrf_raw_demodulator_process and nrf_fm_demodulator_process: `who` is the name in the message */
static void demodulate_f64(const char *who, void *backend, double **audio, int *audio_length, double *samples_i,
                           double *samples_q, int length) {
    fsea_demod *b = (fsea_demod *)backend;
    audio_buffer(b, audio, audio_length, length);
    const int rc = fsea_demod_f64_host(b, samples_i, samples_q, (size_t)length, *audio);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, who, rc);
}

/* the reference's constructors without the backend: nrf_decoder_new owns one of its own */
static nrf_raw_demodulator *raw_shell(int in_sample_rate, int out_sample_rate) {
    nrf_raw_demodulator *d = (nrf_raw_demodulator *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_raw_demodulator));
    d->in_sample_rate = in_sample_rate;
    d->out_sample_rate = out_sample_rate;
    d->downsampler_audio = nrf_downsampler_new(in_sample_rate, out_sample_rate, out_sample_rate / 2, 41);
    return d;
}

static nrf_fm_demodulator *fm_shell(int in_sample_rate, int out_sample_rate) {
    nrf_fm_demodulator *d = (nrf_fm_demodulator *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_fm_demodulator));
    const double filter_freq = FM_MAX_F * 0.8;
    d->in_sample_rate = in_sample_rate;
    d->out_sample_rate = out_sample_rate;
    d->ampl_conv = out_sample_rate / (TAU * FM_MAX_F);
    d->downsampler_i = nrf_downsampler_new(in_sample_rate, FM_INTER_RATE, (int)filter_freq, 51);
    d->downsampler_q = nrf_downsampler_new(in_sample_rate, FM_INTER_RATE, (int)filter_freq, 51);
    d->downsampler_audio = nrf_downsampler_new(FM_INTER_RATE, out_sample_rate, 10000, 41);
    return d;
}

/* ---- RAW demodulator ------------------------------------------------------------- */

nrf_raw_demodulator *nrf_raw_demodulator_new(int in_sample_rate, int out_sample_rate) {
    nrf_raw_demodulator *d = raw_shell(in_sample_rate, out_sample_rate);
    d->backend = backend_new(FSEA_DEMOD_RAW, in_sample_rate, out_sample_rate);
    return d;
}

void nrf_raw_demodulator_process(nrf_raw_demodulator *demodulator, double *samples_i, double *samples_q, int length) {
    demodulate_f64("nrf_raw_demodulator_process", demodulator->backend, &demodulator->audio_samples,
                   &demodulator->audio_samples_length, samples_i, samples_q, length);
}

void nrf_raw_demodulator_free(nrf_raw_demodulator *demodulator) {
    if (demodulator == NULL) return;
    backend_free(demodulator->backend);
    nrf_downsampler_free(demodulator->downsampler_audio);
    free(demodulator->audio_samples);
    free(demodulator);
}

/* ---- WBFM demodulator ------------------------------------------------------------ */

nrf_fm_demodulator *nrf_fm_demodulator_new(int in_sample_rate, int out_sample_rate) {
    nrf_fm_demodulator *d = fm_shell(in_sample_rate, out_sample_rate);
    d->backend = backend_new(FSEA_DEMOD_WBFM, in_sample_rate, out_sample_rate);
    return d;
}

void nrf_fm_demodulator_process(nrf_fm_demodulator *demodulator, double *samples_i, double *samples_q, int length) {
    demodulate_f64("nrf_fm_demodulator_process", demodulator->backend, &demodulator->audio_samples,
                   &demodulator->audio_samples_length, samples_i, samples_q, length);
}

void nrf_fm_demodulator_free(nrf_fm_demodulator *demodulator) {
    if (demodulator == NULL) return;
    backend_free(demodulator->backend);
    nrf_downsampler_free(demodulator->downsampler_i);
    nrf_downsampler_free(demodulator->downsampler_q);
    nrf_downsampler_free(demodulator->downsampler_audio);
    free(demodulator->demodulated_samples);
    free(demodulator->audio_samples);
    free(demodulator);
}

/* ---- Decoder ----------------------------------------------------------------------- */

nrf_decoder *nrf_decoder_new(nrf_demodulate_type demodulate_type, int in_sample_rate, int out_sample_rate, int freq_offset) {
    nrf_decoder *decoder = (nrf_decoder *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_decoder));
    decoder->in_sample_rate = in_sample_rate;
    decoder->out_sample_rate = out_sample_rate;
    decoder->demodulate_type = demodulate_type;
    if (demodulate_type == NRF_DEMODULATE_RAW) {
        decoder->demodulator = raw_shell(in_sample_rate, out_sample_rate);
        decoder->backend = backend_new(FSEA_DEMOD_RAW, in_sample_rate, out_sample_rate);
    } else if (demodulate_type == NRF_DEMODULATE_WBFM) {
        decoder->demodulator = fm_shell(in_sample_rate, out_sample_rate);
        decoder->backend = backend_new(FSEA_DEMOD_WBFM, in_sample_rate, out_sample_rate);
    }
    decoder->freq_shifter = nrf_freq_shifter_new(freq_offset, in_sample_rate);
    if (decoder->freq_shifter == NULL) nrf_private_oom(BLOCK);
    return decoder;
}

/* the (audio_samples, audio_samples_length) pair of the decoder's demodulator, of either type */
static void decoder_audio(nrf_decoder *decoder, double ***audio, int **audio_length) {
    if (decoder->demodulate_type == NRF_DEMODULATE_RAW) {
        nrf_raw_demodulator *d = (nrf_raw_demodulator *)decoder->demodulator;
        *audio = &d->audio_samples;
        *audio_length = &d->audio_samples_length;
    } else {
        nrf_fm_demodulator *d = (nrf_fm_demodulator *)decoder->demodulator;
        *audio = &d->audio_samples;
        *audio_length = &d->audio_samples_length;
    }
}

/* no demodulator: the phase advances as the reference's nrf_freq_shifter_process_samples would advance it */
static void advance_phase_only(nrf_freq_shifter *fs, size_t length) {
    const double delta_cos = cos(TAU * fs->freq_offset / (double)fs->sample_rate);
    const double delta_sin = sin(TAU * fs->freq_offset / (double)fs->sample_rate);
    double cosine = fs->cosine, sine = fs->sine;
    for (size_t i = 0; i < length; i++) {
        const double new_sine = cosine * delta_sin + sine * delta_cos;
        const double new_cosine = cosine * delta_cos - sine * delta_sin;
        sine = new_sine;
        cosine = new_cosine;
    }
    fs->cosine = cosine;
    fs->sine = sine;
}

void nrf_decoder_process(nrf_decoder *decoder, uint8_t *buffer, size_t length) {
    nrf_freq_shifter *fs = decoder->freq_shifter;
    fsea_demod *b = (fsea_demod *)decoder->backend;
    if (b == NULL) {
        advance_phase_only(fs, length);
        return;
    }
    int rc = fsea_demod_set_channel(b, 0, fs->freq_offset, fs->cosine, fs->sine);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_demod_set_channel", rc);
    double **audio;
    int *audio_length;
    decoder_audio(decoder, &audio, &audio_length);
    audio_buffer(b, audio, audio_length, (int)length);
    rc = fsea_demod_u8_host(b, buffer, length, 0, *audio);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "nrf_decoder_process", rc);
    rc = fsea_demod_get_channel(b, 0, NULL, &fs->cosine, &fs->sine);
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_demod_get_channel", rc);
    decoder->audio_samples = *audio;
    decoder->audio_samples_length = *audio_length;
}

void nrf_decoder_free(nrf_decoder *decoder) {
    if (decoder == NULL) return;
    backend_free(decoder->backend);
    if (decoder->demodulate_type == NRF_DEMODULATE_RAW) {
        nrf_raw_demodulator_free((nrf_raw_demodulator *)decoder->demodulator);
    } else if (decoder->demodulate_type == NRF_DEMODULATE_WBFM) {
        nrf_fm_demodulator_free((nrf_fm_demodulator *)decoder->demodulator);
    }
    nrf_freq_shifter_free(decoder->freq_shifter);
    free(decoder);
}
