/* nut_private.h -- helpers shared inside libfsea_nrf.so, not part of the nut.h interface. */
#ifndef FSEA_NUT_PRIVATE_H
#define FSEA_NUT_PRIVATE_H

#include "nut.h"

/* F64 buffer (length x channels) whose payload is NOT zero-filled: for callers that overwrite every
 * element at once (nrf_fft_get_buffer linearising its ring). */
nut_buffer *nut_private_new_f64_unfilled(int n_elements, int n_channels);

/* nrf_iq_draw.c, shared with nrf_iq_chain.c: the points nrf_buffer_to_iq_lines joins for a buffer of `size` elements and a
 * line_percentage (the reference's clamp and float product), and its print-and-exit check of a size_multiplier. */
int nrf_private_iq_line_points(int size, float line_percentage);
void nrf_private_check_iq_multiplier(int size_multiplier);

#endif
