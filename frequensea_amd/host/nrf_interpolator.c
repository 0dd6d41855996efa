/*
 * nrf_interpolator.c -- frequensea's interpolator block (include/nrf.h): a linear cross-fade from one sample block to the
 * next, one step per call.
 *
 * Reference behaviour restated (paths under the reference tree): src/nrf.c:442-496.
 *   nrf_interpolator_process     the reference's state machine on t, including its `else` without braces: t advances only
 *                       on a call that neither starts nor swaps, and such a call ignores its buffer.  The two blocks live
 *                       on the GPU (fsea_interp_*, include/fsea.h); a start or a swap uploads the one new block
 *   nrf_interpolator_get_buffer  one blended frame at weight t from the GPU (fsea_interp_frames_host)
 * Differences: buffer_a and buffer_b stay NULL (the blocks are device memory); get_buffer before the first process, and a
 * later buffer of another type or size, print and exit (the reference dereferences NULL / trips an assert), as does a
 * backend failure (no GPU).  The backend is created by the first process call, which fixes type and size, on the device
 * NRF_FFT_DEVICE names.
 */
#include <stdio.h>
#include <stdlib.h>

#include "fsea.h"
#include "nrf.h"
#include "nrf_private.h"

#define BLOCK "interpolator"

typedef struct {
    fsea_interp *interp;
    nut_buffer_type type;
    int length, channels;
} interp_backend;

static void push(interp_backend *b, const nut_buffer *buffer) {
    if (buffer->type != b->type || buffer->length * buffer->channels != b->length * b->channels) {
        fprintf(stderr, "NRF interpolator fatal error: a buffer of type %d with %d elements follows type %d with %d\n",
                (int)buffer->type, buffer->length * buffer->channels, (int)b->type, b->length * b->channels);
        exit(EXIT_FAILURE);
    }
    const int rc = fsea_interp_push_host(b->interp, nrf_private_payload(buffer));
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_interp_push_host", rc);
}

nrf_interpolator *nrf_interpolator_new(double interpolate_step) {
    nrf_interpolator *interpolator = (nrf_interpolator *)nrf_private_calloc(BLOCK, 1, sizeof(nrf_interpolator));
    interpolator->interpolate_step = interpolate_step;
    interpolator->t = -1;
    return interpolator;
}

void nrf_interpolator_process(nrf_interpolator *interpolator, nut_buffer *buffer) {
    if (interpolator->t < 0.0) {
        /* start: A is zeros (a fresh backend), B the buffer */
        interp_backend *b = (interp_backend *)nrf_private_calloc(BLOCK, 1, sizeof(interp_backend));
        const int size = buffer->length * buffer->channels;
        if (size < 0) {
            fprintf(stderr, "NRF interpolator fatal error: negative buffer size\n");
            exit(EXIT_FAILURE);
        }
        b->type = buffer->type;
        b->length = buffer->length;
        b->channels = buffer->channels;
        const int rc = fsea_interp_create(&b->interp, buffer->type == NUT_BUFFER_U8 ? FSEA_IQ_U8 : FSEA_IQ_F64, (size_t)size,
                                          nrf_private_device());
        if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_interp_create", rc);
        interpolator->backend = b;
        push(b, buffer);
        interpolator->t = 0.0;
    } else if (interpolator->t >= 1.0) {
        /* swap: A takes what B held, B the buffer */
        push((interp_backend *)interpolator->backend, buffer);
        interpolator->t = 0.0;
    } else {
        /* the reference's increment hangs on its `else`: only a call that neither starts nor swaps advances t */
        interpolator->t += interpolator->interpolate_step;
    }
}

nut_buffer *nrf_interpolator_get_buffer(nrf_interpolator *interpolator) {
    interp_backend *b = (interp_backend *)interpolator->backend;
    if (b == NULL) {
        fprintf(stderr, "NRF interpolator fatal error: nrf_interpolator_get_buffer before the first nrf_interpolator_process\n");
        exit(EXIT_FAILURE);
    }
    nut_buffer *dst = b->type == NUT_BUFFER_U8 ? nut_buffer_new_u8(b->length, b->channels, NULL)
                                                : nut_buffer_new_f64(b->length, b->channels, NULL);
    const double t = interpolator->t;
    const int rc = fsea_interp_frames_host(b->interp, &t, 1, nrf_private_payload(dst));
    if (rc != FSEA_OK) nrf_private_fatal(BLOCK, "fsea_interp_frames_host", rc);
    return dst;
}

void nrf_interpolator_free(nrf_interpolator *interpolator) {
    if (interpolator == NULL) return;
    interp_backend *b = (interp_backend *)interpolator->backend;
    if (b != NULL) {
        fsea_interp_destroy(b->interp);
        free(b);
    }
    free(interpolator);
}
