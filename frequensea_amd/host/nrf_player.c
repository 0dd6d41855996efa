/*
 * nrf_player.c -- frequensea's audio player (include/nrf.h) without an audio device.
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:1096-1280.  Each block the device delivers
 * is decoded (nrf_decoder_process, 48 kHz) and converted to (int16_t)(audio * 32000); the reference hands that PCM to
 * OpenAL, this build queues it (nrf_player_pop_pcm) and, with NRF_PLAYER_PCM=<path>, appends it to a raw s16le file.
 * Differences: no OpenAL; device->samples is copied under data_mutex before decoding (the reference reads it unlocked);
 * nrf_player_free waits for a decode in flight (nrf_device_set_decode_handler returns only after it); set_gain stores
 * the clamped gain.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "player"

static const int AUDIO_SAMPLE_RATE = 48000;

static float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

static void player_decode(nrf_device *device, void *ctx) {
    nrf_player *player = (nrf_player *)ctx;
    if (player->shutting_down) return;
    uint8_t *block = (uint8_t *)nrf_private_malloc(BLOCK, NRF_BUFFER_SIZE_BYTES);
    pthread_mutex_lock(&device->data_mutex);
    memcpy(block, device->samples, NRF_BUFFER_SIZE_BYTES);
    pthread_mutex_unlock(&device->data_mutex);

    nrf_decoder_process(player->decoder, block, NRF_SAMPLES_LENGTH);
    free(block);
    const double *audio = player->decoder->audio_samples;
    const int length = audio ? player->decoder->audio_samples_length : 0;
    int16_t *pcm = (int16_t *)nrf_private_malloc(BLOCK, sizeof(int16_t) * (size_t)(length > 0 ? length : 1));
    for (int i = 0; i < length; i++) pcm[i] = (int16_t)(audio[i] * 32000);

    if (player->pcm_file != NULL && length > 0) {
        fwrite(pcm, sizeof(int16_t), (size_t)length, (FILE *)player->pcm_file);
        fflush((FILE *)player->pcm_file);
    }
    pthread_mutex_lock(&player->mutex);
    if (player->queue_size == NRF_PLAYER_QUEUE) { /* full: drop the oldest */
        free(player->queue[player->queue_head]);
        player->queue_head = (player->queue_head + 1) % NRF_PLAYER_QUEUE;
        player->queue_size--;
    }
    const int slot = (player->queue_head + player->queue_size) % NRF_PLAYER_QUEUE;
    player->queue[slot] = pcm;
    player->queue_length[slot] = length;
    player->queue_sequence[slot] = player->next_sequence++;
    player->queue_size++;
    pthread_mutex_unlock(&player->mutex);
}

nrf_player *nrf_player_new(nrf_device *device, nrf_demodulate_type demodulate_type, int freq_offset) {
    nrf_player *player = (nrf_player *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_player));
    player->demodulate_type = demodulate_type;
    player->device = device;
    player->decoder = nrf_decoder_new(demodulate_type, device->sample_rate, AUDIO_SAMPLE_RATE, freq_offset);
    player->gain = 1.0f;
    pthread_mutex_init(&player->mutex, NULL);
    const char *path = getenv("NRF_PLAYER_PCM");
    if (path != NULL && path[0] != '\0') {
        player->pcm_file = fopen(path, "ab");
        if (player->pcm_file == NULL) fprintf(stderr, "WARN nrf_player_new: cannot open %s for PCM\n", path);
    }
    nrf_device_set_decode_handler(device, player_decode, player);
    return player;
}

void nrf_player_set_freq_offset(nrf_player *player, int freq_offset) {
    player->decoder->freq_shifter->freq_offset = freq_offset;
}

void nrf_player_set_gain(nrf_player *player, float gain) { player->gain = clampf(gain, 0.0f, 1.0f); }

int nrf_player_pop_pcm(nrf_player *player, int16_t *out, int capacity, long *sequence) {
    pthread_mutex_lock(&player->mutex);
    if (player->queue_size == 0) {
        pthread_mutex_unlock(&player->mutex);
        return 0;
    }
    const int slot = player->queue_head;
    int16_t *pcm = player->queue[slot];
    const int length = player->queue_length[slot];
    if (sequence != NULL) *sequence = player->queue_sequence[slot];
    player->queue[slot] = NULL;
    player->queue_head = (slot + 1) % NRF_PLAYER_QUEUE;
    player->queue_size--;
    pthread_mutex_unlock(&player->mutex);
    if (out != NULL && capacity > 0) memcpy(out, pcm, sizeof(int16_t) * (size_t)(length < capacity ? length : capacity));
    free(pcm);
    return length;
}

void nrf_player_free(nrf_player *player) {
    if (player == NULL) return;
    player->shutting_down = 1;
    /* returns after a decode in flight has finished: nothing of the player is used after this */
    nrf_device_set_decode_handler(player->device, NULL, NULL);
    /* we don't own the device, so it is not freed */
    nrf_decoder_free(player->decoder);
    for (int i = 0; i < player->queue_size; i++) free(player->queue[(player->queue_head + i) % NRF_PLAYER_QUEUE]);
    if (player->pcm_file != NULL) fclose((FILE *)player->pcm_file);
    pthread_mutex_destroy(&player->mutex);
    free(player);
}
