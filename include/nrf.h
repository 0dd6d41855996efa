/*
 * nrf.h -- the part of frequensea's SDR block library that sits on the
 * IQ-FFT path, with the spectrum computed on an MI355X instead of by FFTW.
 *
 * Interface being replaced (paths under /root/reference):
 *   src/nrf.h:19-23    NRF_* constants
 *   src/nrf.h:25-52    nrf_block + NRF_BLOCK (must stay the FIRST member of
 *                      every block struct: src/main.cpp:616-624 reads
 *                      block->type through the Lua table's __ptr__)
 *   src/nrf.h:56-103   nrf_device (file-replay "dummy" source only; the
 *                      HackRF / RTL-SDR drivers are out of scope)
 *   src/nrf.h:128-142  nrf_fft: nrf_fft_new / _shift / _process /
 *                      _get_buffer / _free -- identical signatures
 *   src/nrf.h:192-207  nrf_freq_shifter, the block lua/fft-shifted.lua puts in
 *                      front of nrf_fft (host arithmetic, as in the reference)
 *   src/nrf.h:145-175  nrf_fir_filter (host, double, as in the reference) and
 *                      nrf_iq_filter, whose convolution runs on the GPU
 *                      (fsea_fir_*, include/fsea.h)
 *   src/nrf.h:100-101, 122-124, 209-218  the IQ drawing functions, whose
 *                      per-sample loops run on the GPU (fsea_iq_*, include/fsea.h),
 *                      and the signal detector (host, double)
 *   src/nrf.h:177-190, 220-301  the downsampler (host, double), the RAW and
 *                      WBFM demodulators and the decoder, whose chains run on
 *                      the GPU (fsea_demod_*, include/fsea.h), and the player
 *                      without OpenAL (a PCM queue and an optional s16le file)
 * Differences, all invisible to callers: <fftw3.h> is gone, the FFTW-typed
 * members of nrf_fft (touched by nobody outside src/nrf.c) became an opaque
 * backend handle, the history is a ring instead of an 8 MiB memmove per row,
 * and a mutex serialises process / get_buffer / shift (the reference has a
 * latent race there: src/nrf.c:37-50 vs src/main.cpp:801).
 *
 * Error convention as in the reference (src/nrf.c:54-78): these functions do
 * not return status codes; a fatal backend error (no GPU, HIP failure) prints
 * to stderr and exit(EXIT_FAILURE)s.  There is no CPU fallback.
 */
#ifndef NRF_H
#define NRF_H

#include <pthread.h>
#include <stdint.h>

#include "nut.h"

#define NRF_BUFFER_SIZE_BYTES (16 * 16384) /* one device block: 262144 bytes */
#define NRF_SAMPLES_LENGTH 131072          /* IQ samples per block */
#define NRF_IQ_RESOLUTION 256
#define DEFAULT_FFT_SIZE 128
#define DEFAULT_FFT_HISTORY_SIZE 128

/* ---- block graph (src/nrf.h:25-52, src/nrf.c:24-50) ------------------- */

#define NRF_BLOCK_MAX_OUTPUTS 10

typedef enum {
    NRF_BLOCK_SOURCE = 1,
    NRF_BLOCK_GENERIC,
    NRF_BLOCK_SINK
} nrf_block_type;

typedef struct nrf_block nrf_block;
typedef void (*nrf_block_process_fn)(nrf_block *block, nut_buffer *buffer);
typedef nut_buffer *(*nrf_block_result_fn)(void *block);

struct nrf_block {
    nrf_block_type type;
    nrf_block_process_fn process_fn;
    nrf_block_result_fn result_fn;
    int n_outputs;
    void *outputs[NRF_BLOCK_MAX_OUTPUTS];
};

void nrf_block_init(nrf_block *block, nrf_block_type type, nrf_block_process_fn process_fn,
                    nrf_block_result_fn result_fn);
void nrf_block_connect(nrf_block *input, nrf_block *output);
/* process_fn(block, buffer); then, if the block has outputs, push result_fn's
 * buffer to each of them and free it. */
void nrf_block_process(nrf_block *block, nut_buffer *buffer);

#define NRF_BLOCK nrf_block block

/* ---- sample source (src/nrf.h:56-103) ---------------------------------- */

typedef struct {
    int sample_rate;
    double freq_mhz;
    const char *data_file;
} nrf_device_config;

typedef enum {
    NRF_DEVICE_DUMMY = 0,
    NRF_DEVICE_RTLSDR,
    NRF_DEVICE_HACKRF
} nrf_device_type;

typedef struct nrf_device nrf_device;
typedef void (*nrf_device_decode_cb_fn)(nrf_device *device, void *ctx);

struct nrf_device {
    NRF_BLOCK;
    nrf_device_type device_type; /* always NRF_DEVICE_DUMMY in this build */
    void *device;
    int sample_rate;

    nrf_device_decode_cb_fn decode_cb_fn;
    void *decode_cb_ctx;

    pthread_t receive_thread;
    pthread_mutex_t data_mutex;
    int receiving;
    int paused;

    uint8_t *receive_buffer; /* whole replay file, raw HackRF int8 bytes */
    int dummy_block_length;  /* blocks in receive_buffer */
    int dummy_block_index;

    uint8_t samples[NRF_BUFFER_SIZE_BYTES]; /* current block, offset binary */

    /* this build: held while the replay thread runs the decode handler and while nrf_device_set_decode_handler swaps it,
     * so that once set_decode_handler returns no call of the previous handler is still running */
    pthread_mutex_t decode_mutex;
};

/* Replays `data_file` (raw int8 IQ as written by c/rfcap.c) in 262144-byte
 * blocks at 60 Hz on its own thread, flipping each byte to offset binary
 * (src/nrf.c:95-110, 162-170, 256-284).  A missing file gives one zero block. */
nrf_device *nrf_device_new(double freq_mhz, const char *data_file);
nrf_device *nrf_device_new_with_config(nrf_device_config config);
double nrf_device_set_frequency(nrf_device *device, double freq_mhz);
void nrf_device_set_decode_handler(nrf_device *device, nrf_device_decode_cb_fn fn, void *ctx);
void nrf_device_set_paused(nrf_device *device, int paused);
void nrf_device_step(nrf_device *device);
/* Locked snapshot: u8, length NRF_SAMPLES_LENGTH, 2 channels (src/nrf.c:352-357). */
nut_buffer *nrf_device_get_samples_buffer(nrf_device *device);
/* The IQ images of the current block (src/nrf.c:359-372, 399-421): nrf_buffer_to_iq_points / _iq_lines (below) on all
 * NRF_BUFFER_SIZE_BYTES of device->samples.  The block is copied under data_mutex, which is released before the GPU
 * draws (the reference holds it throughout). */
nut_buffer *nrf_device_get_iq_buffer(nrf_device *device);
nut_buffer *nrf_device_get_iq_lines(nrf_device *device, int size_multiplier, float line_percentage);
void nrf_device_free(nrf_device *device);

/* ---- interpolator (src/nrf.h:105-118, src/nrf.c:442-496) ----------------- */

/* A linear cross-fade between consecutive blocks, t in interpolate_step steps.  The reference's members keep their order
 * and types; the backend handle is appended.  The two blocks live on the device: buffer_a and buffer_b are kept as
 * members and stay NULL.  The block member is zeroed and never initialised, as in the reference. */
typedef struct {
    NRF_BLOCK;
    double interpolate_step;
    double t;
    nut_buffer *buffer_a;
    nut_buffer *buffer_b;
    void *backend; /* the two device blocks (fsea_interp*, libfsea_hip.so) with their type and shape; NULL before the first process */
} nrf_interpolator;

/* t = -1, no blocks yet. */
nrf_interpolator *nrf_interpolator_new(double interpolate_step);
/* The reference's state machine, its `else` without braces included (src/nrf.c:451-468): the first call fixes type and
 * size, A = zeros, B = buffer, t = 0; a call with t >= 1.0 makes A what B was, B = buffer, t = 0; any other call adds
 * interpolate_step to t AND IGNORES ITS BUFFER.  A later buffer of another type or size prints and exits (the reference
 * asserts), as does a backend failure (no GPU). */
void nrf_interpolator_process(nrf_interpolator *interpolator, nut_buffer *buffer);
/* Fresh buffer of A's type, length and channels: a (1.0 - t) + b t per element in double (u8: through / 256.0 and
 * (uint8_t)(v * 256.0), as nut_buffer_get_f64 / nut_buffer_set_f64); caller frees with nut_buffer_free.  Before the first
 * process: prints and exits (the reference dereferences NULL). */
nut_buffer *nrf_interpolator_get_buffer(nrf_interpolator *interpolator);
void nrf_interpolator_free(nrf_interpolator *interpolator);

/* ---- FFT analysis (src/nrf.h:128-142, src/nrf.c:557-642) ---------------- */

typedef struct {
    NRF_BLOCK;
    int fft_size;
    int fft_history_size;
    double *buffer;        /* history ring: fft_history_size rows of fft_size */
    int ring_head;         /* ring row that holds the newest spectrum */
    void *backend;         /* fsea_plan* (libfsea_hip.so) */
    float *row_f32;        /* staging for one device row */
    void *scratch;         /* zero-padded / converted input for short buffers */
    pthread_mutex_t mutex;
    void *device_history;  /* fsea_history* when NRF_FFT_HISTORY=device: the ring lives in HBM, `buffer` is NULL */
} nrf_fft;

/* Plan + zeroed history of fft_history_size rows.  Exits if no GPU. */
nrf_fft *nrf_fft_new(int fft_size, int fft_history_size);
/* Scroll every history row by round(fft_size / d) bins (src/nrf.c:569-596). */
void nrf_fft_shift(nrf_fft *fft, double d);
/* One new row from the first fft_size samples of `buffer` (u8 IQ as produced by
 * nrf_device_get_samples_buffer, or f64 IQ): x[n] = (-1)^n * u8/256, forward
 * DFT, magnitude, bin N/2 := bin N/2-1; pushed as row 0 (src/nrf.c:598-631). */
void nrf_fft_process(nrf_fft *fft, nut_buffer *buffer);
/* Fresh f64 copy of the whole history, newest row first; caller frees with
 * nut_buffer_free (src/nrf.c:633-635). */
nut_buffer *nrf_fft_get_buffer(nrf_fft *fft);
void nrf_fft_free(nrf_fft *fft);
/* ADDITIONS (not in the reference; the five prototypes above are src/nrf.h:138-142 unchanged).  BASELINE's north_star
 * names a "windowed 1D FFT"; the reference's only pre-FFT weight is powf(-1, ii) (src/nrf.c:611-612), i.e. rectangular.
 * A taper w[n] rides beside that sign in the kernel's fused unpack prologue: x[n] = (-1)^n w[n] u8[n]/256 (fsea.h:
 * fsea_plan_set_window).  Per nrf_fft object; callable at any time, also between nrf_fft_process calls and from another
 * thread (taken under the block's mutex): rows already in the history keep the taper they were computed with.
 *   name: "hann", "hamming", "blackman", "blackmanharris", "flattop" (periodic, scipy.signal.get_window's values), or
 *         "rect" / "none" / "" / NULL = the reference's rectangular frames.  Anything else: message on stderr + exit, the
 *         reference's convention for a wrong argument (src/main.cpp:46-60).
 *   weights: fft_size floats, copied; NULL = rectangular.
 * The environment variable NRF_FFT_WINDOW=<name> is the default every nrf_fft_new starts from (unmodified scenes). */
void nrf_fft_set_window(nrf_fft *fft, const char *name);
void nrf_fft_set_window_weights(nrf_fft *fft, const float *weights);

/* ---- frequency shifter (src/nrf.h:192-207, src/nrf.c:817-870) ------------ */

typedef struct {
    NRF_BLOCK;
    int freq_offset; /* Hz */
    int sample_rate; /* Hz */
    double cosine;   /* phase carried from block to block, starts at (1, 0) */
    double sine;
    nut_buffer *buffer; /* last output, F64 */
} nrf_freq_shifter;

nrf_freq_shifter *nrf_freq_shifter_new(int freq_offset, int sample_rate);
/* In place on separate I and Q arrays: (i, q) <- (i, q) rotated by the running phase, which
 * advances by 2 pi freq_offset / sample_rate per sample.  No offset is added. */
void nrf_freq_shifter_process_samples(nrf_freq_shifter *shifter, double *samples_i, double *samples_q, int length);
/* Interleaved 2-channel buffer (u8 values count as u8 / 256.0): rotated samples + 0.5 on both
 * components go to the shifter's own F64 buffer.  As in the reference that buffer is created with
 * length = buffer->length * 2 and 2 channels, i.e. twice the room it needs; only the first half is
 * written (src/nrf.c:851).  nrf_fft_process reads just the first fft_size samples of it. */
void nrf_freq_shifter_process(nrf_freq_shifter *shifter, nut_buffer *buffer);
/* Copy of the last output (NULL before the first process call). */
nut_buffer *nrf_freq_shifter_get_buffer(nrf_freq_shifter *shifter);
void nrf_freq_shifter_free(nrf_freq_shifter *shifter);

/* ---- FIR filter and IQ filter (src/nrf.h:145-175, src/nrf.c:654-775) ---- */

/* The per-sample pull filter, on the host in double, bit for bit the reference's.  `length` taps are used of the
 * length + (length + 1) % 2 designed ones (an even length: an asymmetric filter that does not sum to 1, as in the
 * reference); `samples` holds the last offset = length - 1 samples of the previous loads followed by the last load. */
typedef struct {
    int length;
    double *coefficients;
    int offset;
    int center;
    int samples_length;
    double *samples;
} nrf_fir_filter;

/* malloc'd array of length + (length + 1) % 2 taps (window-method low-pass, normalised to sum 1). */
double *nrf_fir_get_low_pass_coefficients(int sample_rate, int half_ampl_freq, int length);
nrf_fir_filter *nrf_fir_filter_new(int sample_rate, int half_ampl_freq, int length);
void nrf_fir_filter_load(nrf_fir_filter *filter, double *samples, int length);
/* sum_{i < length} coefficients[i] * samples[index + i]: output `index` of the last load. */
double nrf_fir_filter_get(nrf_fir_filter *filter, int index);
void nrf_fir_filter_free(nrf_fir_filter *filter);

/* The IQ low-pass filter: I and Q through the same taps, state carried from call to call, the convolution on the GPU in
 * f32 (fsea_fir_*: one kernel launch per process call).  kernel_length must lie in [1, FSEA_FIR_MAX_TAPS] (512): anything
 * else prints and exits, as does a backend failure (no GPU).  The reference keeps two nrf_fir_filter and the de-interleaved
 * input here; this block keeps the backend object and the last call's output instead. */
typedef struct {
    NRF_BLOCK;
    int length;          /* taps */
    int samples_length;  /* IQ pairs of the last process call (the length of the next get_buffer) */
    void *backend;       /* fsea_fir* (libfsea_hip.so) */
    float *output;       /* the last call's samples_length filtered (I, Q) pairs */
    int output_capacity; /* pairs */
    pthread_mutex_t mutex;
} nrf_iq_filter;

nrf_iq_filter *nrf_iq_filter_new(int sample_rate, int half_ampl_freq, int kernel_length);
/* Filters buffer->length IQ pairs (u8 values count as u8 / 256.0, f64 as is; 2 channels). */
void nrf_iq_filter_process(nrf_iq_filter *filter, nut_buffer *buffer);
/* Fresh F64 buffer of the last call's length with 2 channels, interleaved I, Q; length 0 before any process call. */
nut_buffer *nrf_iq_filter_get_buffer(nrf_iq_filter *f);
void nrf_iq_filter_free(nrf_iq_filter *filter);

/* ---- IQ drawing (src/nrf.h:122-124, src/nrf.c:499-553) ---- */

/* A copy of `buffer` with one channel more: after each group of `channels` elements, t = i / (double)size, i the group's
 * first element and size = length * channels.  Host arithmetic (nut_buffer_get_f64 / _set_f64: a U8 result holds
 * (uint8_t)(t * 256.0)). */
nut_buffer *nrf_buffer_add_position_channel(nut_buffer *buffer);
/* The 256 x 256 U8 point histogram (length 65536, 1 channel) of the length * channels elements of `buffer` read pairwise
 * as (I, Q) whatever its channel count (an incomplete last pair is ignored), coordinates by nut_buffer_get_u8; bin
 * I * 256 + Q, each pair adding 1 modulo 256 as the reference's u8++.  Drawn on the GPU (fsea_iq_points_host). */
nut_buffer *nrf_buffer_to_iq_points(nut_buffer *buffer);
/* The (256 m)^2 U8 line image, m = size_multiplier: line_percentage is clamped to [0, 1] (a NaN draws nothing), the
 * points at elements i = 0, 2, ... < (int)((float)size * line_percentage) are joined by the reference's draw_line
 * (Bresenham, both endpoints included) from each to the next, pixel (I m, Q m) at Q m * 256 m + I m (transposed relative
 * to the points image), each pixel saturating at 255.  Drawn on the GPU (fsea_iq_lines_host).  Deliberate difference: a
 * size_multiplier outside [1, FSEA_IQ_MAX_MULTIPLIER] (16) prints and exits; the reference would allocate an image of
 * zero or negative size.  Both functions return a fresh buffer that the caller frees. */
nut_buffer *nrf_buffer_to_iq_lines(nut_buffer *buffer, int size_multiplier, float line_percentage);

/* ---- ADDITIONS (not in the reference): the IQ chain ---- */

/* What the reference's IQ scenes do per block with three blocks and two drawing calls, as one block whose data stays on
 * the GPU: [nrf_freq_shifter ->] nrf_iq_filter -> nrf_buffer_to_iq_points / nrf_buffer_to_iq_lines (lua/dvbt.lua:46-51,
 * lua/iq-tex-filtered.lua:44-47).  process uploads the 8-bit block (2 bytes per pair), rotates it in the filter kernel's
 * load and filters it into a device buffer (fsea_chain_*, include/fsea.h); each getter draws from that buffer and brings
 * back its image alone.  The contract is drop-in equivalence with the block sequence, quirks included:
 *   - without a shifter: nrf_iq_filter_process + nrf_iq_filter_get_buffer bit for bit, and the images of
 *     nrf_buffer_to_iq_points / _lines applied to that buffer byte for byte;
 *   - with a shifter: nrf_freq_shifter_process + nrf_freq_shifter_get_buffer in front.  The shifter's buffer has twice the
 *     pairs of its input with the back half 0.0 (src/nrf.c:851) and the filter follows its length, so a call on N pairs
 *     filters N rotated pairs and N zero pairs, get_buffer has 2N pairs and the images are drawn over all of them.  The
 *     phase after M consumed samples is M * freq_offset / sample_rate cycles, M an integer kept here (the reference steps a
 *     (cos, sin) pair; the two agree to ~1e-12 over a scene's run, the filter's f32 arithmetic is ~1e-7).
 * F64 input takes a host-staged path (rotated here in double when a shifter is set, by the phase of the U8 path: M *
 * freq_offset / sample_rate reduced modulo 1 as an exact two-term product, not one rounded product).  A kernel length outside
 * [1, FSEA_FIR_MAX_TAPS] prints and exits, as does a size_multiplier outside [1, FSEA_IQ_MAX_MULTIPLIER] and a backend
 * failure (no GPU).  The getters return NULL before the first process call; their buffers are the caller's to free. */
typedef struct {
    NRF_BLOCK;
    int sample_rate;          /* Hz */
    int length;               /* taps */
    int shifting;             /* != 0 once nrf_iq_chain_set_shifter was called */
    int freq_offset;          /* Hz */
    unsigned long long consumed; /* samples the current shifter has rotated */
    int samples_length;       /* IQ pairs of the last process call's result; -1 before the first */
    void *backend;            /* fsea_chain* (libfsea_hip.so) */
    pthread_mutex_t mutex;
} nrf_iq_chain;

/* The filter of nrf_iq_filter_new(sample_rate, half_ampl_freq, kernel_length), no shifter. */
nrf_iq_chain *nrf_iq_chain_new(int sample_rate, int half_ampl_freq, int kernel_length);
/* Installs a FRESH shifter at phase (1, 0), as dvbt.lua:65-69 does on a key press; the filter keeps its state. */
void nrf_iq_chain_set_shifter(nrf_iq_chain *chain, int freq_offset);
/* One block: buffer->length IQ pairs, 2 channels (u8 values count as u8 / 256.0, f64 as is). */
void nrf_iq_chain_process(nrf_iq_chain *chain, nut_buffer *samples);
/* = nrf_buffer_to_iq_points / nrf_buffer_to_iq_lines of nrf_iq_chain_get_buffer's result */
nut_buffer *nrf_iq_chain_get_iq_points(nrf_iq_chain *chain);
nut_buffer *nrf_iq_chain_get_iq_lines(nrf_iq_chain *chain, int size_multiplier, float line_percentage);
/* The filtered block, F64 with 2 channels, as nrf_iq_filter_get_buffer. */
nut_buffer *nrf_iq_chain_get_buffer(nrf_iq_chain *chain);
void nrf_iq_chain_free(nrf_iq_chain *chain);

/* ---- ADDITIONS (not in the reference): the zoom spectrum ---- */

/* A spectrum of 1 / decimation of the device's bandwidth around freq_offset: what nrf_decoder chains for its audio --
 * nrf_freq_shifter -> nrf_downsampler (rate_mul = decimation, on I and on Q) -> nrf_fft -- as one block whose samples stay on
 * the GPU from the 8-bit upload to the rows (fsea_zoom_*, include/fsea.h).  One bin is sample_rate / (decimation * fft_size)
 * wide: lua/fft-sea.lua's 128 points over 10 MHz are 78 kHz per bin, at decimation 16 they are 4.9 kHz.
 *   - The low-pass is nrf_fir_get_low_pass_coefficients(sample_rate, half_ampl_freq, kernel_length) at the input rate.
 *   - The spectrum moves up by freq_offset, the sign convention of nrf_freq_shifter_new: a signal at +f is centred by
 *     passing -f.  The phase after M consumed samples is M * freq_offset / sample_rate cycles, M an integer kept here.
 *   - Rows are nrf_fft's: magnitudes, the DC bin replaced, bin fft_size / 2 the centre.  A block of `length` pairs gives
 *     length / decimation decimated pairs and (that - fft_size) / fft_size + 1 gapless rows (131072 pairs at decimation 16
 *     and 128 points: 64 rows); decimated pairs that do not fill a row are dropped, the filter's state and the phase carry on
 *     to the next block.  A block whose length is not a multiple of decimation restarts the decimation phase, as the
 *     reference's downsampler does with every block.
 *   - get_buffer is the history: fft_history_size rows of fft_size F64 values, one channel, row 0 the newest (all 0.0 at
 *     the start); when a block yields fft_history_size rows or more its newest fft_history_size remain.
 * process takes a U8 buffer with 2 channels.  An F64 buffer, a kernel length outside [1, FSEA_FIR_MAX_TAPS], a decimation
 * outside [1, FSEA_ZOOM_MAX_DECIMATION], a history size below 1 and a backend failure (no GPU, an fft_size no plan serves)
 * print "NRF zoom FFT fatal error: ..." and exit.  The buffer returned is the caller's to free. */
typedef struct {
    NRF_BLOCK;
    int sample_rate;          /* Hz */
    int freq_offset;          /* Hz */
    int decimation;
    int fft_size;
    int fft_history_size;     /* rows */
    unsigned long long consumed; /* samples rotated since the offset was set */
    double *history;          /* fft_history_size x fft_size, row 0 the newest */
    void *backend;            /* fsea_zoom* (libfsea_hip.so) */
    pthread_mutex_t mutex;
} nrf_zoom_fft;

nrf_zoom_fft *nrf_zoom_fft_new(int sample_rate, int freq_offset, int decimation, int half_ampl_freq, int kernel_length,
                               int fft_size, int fft_history_size);
/* Another centre: the phase restarts at 0 and the filter at a zero tail; the history stays. */
void nrf_zoom_fft_set_freq_offset(nrf_zoom_fft *zoom, int freq_offset);
void nrf_zoom_fft_process(nrf_zoom_fft *zoom, nut_buffer *samples);
nut_buffer *nrf_zoom_fft_get_buffer(nrf_zoom_fft *zoom);
void nrf_zoom_fft_free(nrf_zoom_fft *zoom);

/* ---- ADDITIONS (not in the reference): the filter-bank spectrum ---- */

/* nrf_fft with a polyphase filter bank in front of the transform (fsea_pfb_*, include/fsea.h), a drop-in for nrf_fft in the
 * FFT scenes: fft_size channels, the prototype of fsea_pfb_prototype(fft_size, branch_taps), no oversampling.  Where a
 * rectangular fft_size-point row leaks a tone between two bins into every other bin (-17 dB three bins away), a bin here
 * has the prototype's stop band.
 *   - Rows are nrf_fft's in scale and layout: magnitudes, the DC bin replaced, bin fft_size / 2 the centre.  A block of
 *     `length` pairs gives length / fft_size rows; the last fft_size * branch_taps - 1 samples and the stream position carry
 *     on to the next block, so a row looks back over earlier blocks.
 *   - get_buffer is the history: fft_history_size rows of fft_size F64 values, one channel, row 0 the newest (all 0.0 at
 *     the start); when a block yields fft_history_size rows or more its newest fft_history_size remain.
 * process takes a U8 buffer with 2 channels.  An F64 buffer, an fft_size that is odd or outside [2, FSEA_PFB_MAX_CHANNELS],
 * branch_taps outside [1, FSEA_PFB_MAX_BRANCH_TAPS], a history size below 1 and a backend failure (no GPU) print
 * "NRF PFB FFT fatal error: ..." and exit.  The buffer returned is the caller's to free. */
typedef struct {
    NRF_BLOCK;
    int fft_size;             /* channels */
    int fft_history_size;     /* rows */
    int branch_taps;
    double *history;          /* fft_history_size x fft_size, row 0 the newest */
    void *backend;            /* fsea_pfb* (libfsea_hip.so) */
    pthread_mutex_t mutex;
} nrf_pfb_fft;

nrf_pfb_fft *nrf_pfb_fft_new(int fft_size, int fft_history_size, int branch_taps);
void nrf_pfb_fft_process(nrf_pfb_fft *pfb, nut_buffer *samples);
nut_buffer *nrf_pfb_fft_get_buffer(nrf_pfb_fft *pfb);
void nrf_pfb_fft_free(nrf_pfb_fft *pfb);

/* ---- ADDITIONS (not in the reference): the persistence spectrum ---- */

/* An analyser's persistence display of the device's band (fsea_persist_*, include/fsea.h): how often each of the fft_size
 * bins was at each of 256 levels over all the blocks processed.
 *   - process takes a U8 buffer with 2 channels.  All (length - fft_size) / hop + 1 frames of the block go through a
 *     FSEA_MODE_DB5_U8_DCFIX plan on the device and from there into the object: the block goes up once, no row comes back.
 *     A block shorter than fft_size adds nothing.
 *   - set_window takes the names of nrf_fft_set_window.  set_decay(numerator, denominator): every count is scaled by
 *     numerator / denominator (rounded down) before each block, the phosphor of a running display; none by default.
 *   - get_buffer is the picture under the map given at new (FSEA_PERSIST_MAP_*; full scale = the rows counted): a U8 buffer of
 *     256 * fft_size elements, one channel, the strongest level in the first row -- what
 *     ngl_texture_update(texture, buffer, fft_size, 256) takes.  The buffer returned is the caller's to free.
 * An F64 buffer, an fft_size outside [1, FSEA_PERSIST_MAX_WIDTH] or without a plan, a hop below 1, an unknown map or window
 * name, a decay ratio above 1 or with a zero denominator, and a backend failure (no GPU) print
 * "NRF PERSISTENCE fatal error: ..." and exit. */
typedef struct {
    NRF_BLOCK;
    int fft_size;
    int hop;
    int map;                  /* FSEA_PERSIST_MAP_* */
    unsigned decay_numerator, decay_denominator;
    int device;
    void *plan;               /* fsea_plan* (libfsea_hip.so): (fft_size, hop, FSEA_MODE_DB5_U8_DCFIX) */
    void *backend;            /* fsea_persist* */
    void *d_iq, *d_rows;      /* device memory: the block, its rows */
    size_t iq_cap, rows_cap;
    pthread_mutex_t mutex;
} nrf_persistence;

nrf_persistence *nrf_persistence_new(int fft_size, int hop, int map);
void nrf_persistence_set_window(nrf_persistence *p, const char *name);
void nrf_persistence_set_decay(nrf_persistence *p, unsigned numerator, unsigned denominator);
void nrf_persistence_process(nrf_persistence *p, nut_buffer *buffer);
nut_buffer *nrf_persistence_get_buffer(nrf_persistence *p);
void nrf_persistence_free(nrf_persistence *p);

/* ---- ADDITIONS (not in the reference): the spectrum occupancy ---- */

/* A CFAR detector across the device's band (fsea_cfar_*, include/fsea.h): which of the fft_size bins hold a signal, and how
 * often over all the blocks processed.
 *   - new takes the detector's settings: guard and train cells per side, the offset in levels of the DB5 rows
 *     (FSEA_MODE_DB5_U8_DCFIX, include/fsea.h) and the method (FSEA_CFAR_CA, _GO, _SO).
 *   - process takes a U8 buffer with 2 channels.  All (length - fft_size) / hop + 1 frames of the block go through a
 *     FSEA_MODE_DB5_U8_DCFIX plan on the device and from there into the object: the block goes up once, nothing comes
 *     back.  A block shorter than fft_size adds nothing.
 *   - set_window takes the names of nrf_fft_set_window.
 *   - get_buffer is an F64 buffer of fft_size duty cycles hits[k] / rows, one channel, all 0 before any row.
 *   - get_mask_buffer is the last block's mask: a U8 buffer of frames * fft_size elements, one channel, 255 where frame r had
 *     a detection in bin k; of length 0 before any block and after a block shorter than a frame.
 *   Both buffers are the caller's to free.
 * An F64 buffer, an fft_size outside [1, FSEA_CFAR_MAX_WIDTH] or without a plan, a hop below 1, a guard, train, offset or
 * method that fsea_cfar_set refuses, an unknown window name, and a backend failure (no GPU) print
 * "NRF SPECTRUM OCCUPANCY fatal error: ..." and exit. */
typedef struct {
    NRF_BLOCK;
    int fft_size;
    int hop;
    int device;
    void *plan;               /* fsea_plan* (libfsea_hip.so): (fft_size, hop, FSEA_MODE_DB5_U8_DCFIX) */
    void *backend;            /* fsea_cfar* */
    void *d_iq, *d_rows, *d_mask;   /* device memory: the block, its rows, their mask */
    size_t iq_cap, rows_cap, mask_cap;
    size_t mask_rows;         /* frames of the last block */
    pthread_mutex_t mutex;
} nrf_spectrum_occupancy;

nrf_spectrum_occupancy *nrf_spectrum_occupancy_new(int fft_size, int hop, int guard, int train, int offset, int method);
void nrf_spectrum_occupancy_set_window(nrf_spectrum_occupancy *p, const char *name);
void nrf_spectrum_occupancy_process(nrf_spectrum_occupancy *p, nut_buffer *buffer);
nut_buffer *nrf_spectrum_occupancy_get_buffer(nrf_spectrum_occupancy *p);
nut_buffer *nrf_spectrum_occupancy_get_mask_buffer(nrf_spectrum_occupancy *p);
void nrf_spectrum_occupancy_free(nrf_spectrum_occupancy *p);

/* ---- ADDITIONS (not in the reference): the signal capture ---- */

/* The reference's signal scene (lua/signal-detector.lua:89-133) over a whole recording that stays on the GPU: the detector
 * of nrf_signal_detector_process on every block in one launch, the scene's state machine over the statistics, the blocks of
 * each burst through the filter of nrf_iq_filter_new(sample_rate, half_ampl_freq, kernel_length) and appended, a burst
 * drawn as nrf_buffer_to_iq_lines draws the scene's draw_buffer (fsea_capture_*, include/fsea.h).  The contract is
 * equivalence with the block sequence:
 *   - get_mean is nrf_signal_detector_process's mean bit for bit, get_standard_deviation its standard deviation to within
 *     (n / 2 + 16) 2^-53 relative, n the elements of a block (the reference's own sequential sum is no closer to the exact
 *     value);
 *   - a block with standard deviation > threshold starts or continues a burst; the first block at or below it ends the
 *     burst and is dropped; a NaN is not above the threshold;
 *   - get_burst is nrf_iq_filter_process + nrf_iq_filter_get_buffer over the gated blocks in order, joined by
 *     nut_buffer_append, bit for bit: one filter for the whole life of the object, its tail carried across bursts and scans;
 *   - get_iq_lines is nrf_buffer_to_iq_lines of get_burst's buffer byte for byte.
 * scan takes a U8 buffer with 2 channels; block_length is in IQ pairs and a multiple of 8; a trailing partial block is
 * ignored.  Bursts are numbered from 0 and accumulate over the scans of one object; a burst still open at the end of a scan
 * is continued by the next one.  scan returns the number of bursts so far.  The scene's shader gain and alpha fade are
 * rendering and not part of this.  A kernel length outside [1, FSEA_FIR_MAX_TAPS], a block or burst index out of range, a
 * size_multiplier outside [1, FSEA_IQ_MAX_MULTIPLIER] and a backend failure (no GPU) print and exit.  The buffers returned
 * are the caller's to free. */
typedef struct {
    int sample_rate;   /* Hz */
    int length;        /* taps */
    double threshold;  /* the scene's signal_threshold */
    void *backend;     /* fsea_capture* (libfsea_hip.so) */
    pthread_mutex_t mutex;
} nrf_signal_capture;

nrf_signal_capture *nrf_signal_capture_new(int sample_rate, int half_ampl_freq, int kernel_length, double threshold);
int nrf_signal_capture_scan(nrf_signal_capture *capture, nut_buffer *recording, int block_length);
double nrf_signal_capture_get_mean(nrf_signal_capture *capture, int block);
double nrf_signal_capture_get_standard_deviation(nrf_signal_capture *capture, int block);
/* The burst's filtered pairs, F64 with 2 channels: what the scene's draw_buffer holds. */
nut_buffer *nrf_signal_capture_get_burst(nrf_signal_capture *capture, int burst);
nut_buffer *nrf_signal_capture_get_iq_lines(nrf_signal_capture *capture, int burst, int size_multiplier, float line_percentage);
void nrf_signal_capture_free(nrf_signal_capture *capture);

/* ---- Signal detector (src/nrf.h:209-218, src/nrf.c:876-903): host, double, the reference's layout ---- */

/* process: mean = 2 * (sum of the I elements) / size, standard_deviation = sqrt(sum over all elements of
 * (x - mean)^2 / mean), size = length * channels, elements by nut_buffer_get_f64. */
typedef struct {
    double mean;
    double standard_deviation;
} nrf_signal_detector;

nrf_signal_detector *nrf_signal_detector_new();
void nrf_signal_detector_process(nrf_signal_detector *detector, nut_buffer *buffer);
void nrf_signal_detector_free(nrf_signal_detector *detector);

/* ---- Downsampler (src/nrf.h:177-190, src/nrf.c:778-811): host, double, the reference's loop bit for bit ---- */

/* process: the filter (nrf_fir_filter_new(in_rate, filter_freq, kernel_length)) is loaded with the call's samples;
 * out_length = floor(length / rate_mul), rate_mul = in_rate / (double) out_rate, and output i is
 * nrf_fir_filter_get(filter, floor(t)) with t accumulated (t += rate_mul) from 0 on every call. */
typedef struct {
    int in_rate;
    int out_rate;
    nrf_fir_filter *filter;
    double rate_mul;
    int out_length;
    double *out_samples;
} nrf_downsampler;

nrf_downsampler *nrf_downsampler_new(int in_rate, int out_rate, int filter_freq, int kernel_length);
void nrf_downsampler_process(nrf_downsampler *d, double *samples, int length);
void nrf_downsampler_free(nrf_downsampler *d);

/* ---- Demodulators and decoder (src/nrf.h:220-276, src/nrf.c:904-1094) ---- */

/* The chains run on the GPU in f64 (fsea_demod_*, include/fsea.h; one 1-channel object per demodulator or decoder):
 *   RAW:  the downsampler (in, out, out / 2, 41) on I; Q is not used
 *   WBFM: downsamplers (in, 336000, 60000, 51) on I and Q, the reference's discriminator against the previous stage-1
 *         output (carried, 0 at first), the downsampler (336000, out, 10000, 41), de-emphasis val += alpha (x - val),
 *         alpha = 1 / (1 + out * 50 / 1e6); ampl_conv = out / (2 pi 75000)
 * The reference's members keep their order and types; the backend handle is appended.  Differences, all documented in
 * the intermediate arrays are not kept current (the internal downsamplers are created for their
 * configuration but never run: out_length 0, out_samples NULL; demodulated_samples NULL, demodulated_length 0);
 * l_i, l_q and deemphasis_val live on the device (the members stay 0); a backend failure (no GPU) prints and exits. */
typedef struct {
    int in_sample_rate;
    int out_sample_rate;
    nrf_downsampler *downsampler_audio;
    double *audio_samples;
    int audio_samples_length;
    void *backend; /* fsea_demod* (libfsea_hip.so); NULL inside a decoder, which owns its own */
} nrf_raw_demodulator;

nrf_raw_demodulator *nrf_raw_demodulator_new(int in_sample_rate, int out_sample_rate);
void nrf_raw_demodulator_process(nrf_raw_demodulator *demodulator, double *samples_i, double *samples_q, int length);
void nrf_raw_demodulator_free(nrf_raw_demodulator *demodulator);

typedef struct {
    int in_sample_rate;
    int out_sample_rate;
    double ampl_conv;
    double l_i;
    double l_q;
    double deemphasis_val;
    nrf_downsampler *downsampler_i;
    nrf_downsampler *downsampler_q;
    nrf_downsampler *downsampler_audio;
    double *demodulated_samples;
    int demodulated_length;
    double *audio_samples;
    int audio_samples_length;
    void *backend; /* fsea_demod* (libfsea_hip.so); NULL inside a decoder, which owns its own */
} nrf_fm_demodulator;

nrf_fm_demodulator *nrf_fm_demodulator_new(int in_sample_rate, int out_sample_rate);
void nrf_fm_demodulator_process(nrf_fm_demodulator *demodulator, double *samples_i, double *samples_q, int length);
void nrf_fm_demodulator_free(nrf_fm_demodulator *demodulator);

typedef enum {
    NRF_DEMODULATE_RAW = 0,
    NRF_DEMODULATE_WBFM
} nrf_demodulate_type;

/* process: offset-binary bytes (device->samples) converted as buffer[2i] / 128.0 - 0.995, rotated by the frequency
 * shifter's phase, then RAW or WBFM.  Each call reads freq_shifter->freq_offset / cosine / sine first (callers and the
 * player write them directly) and writes the advanced phase back; the phase of sample k is taken from the exactly reduced
 * cycle count (freq_offset k mod in_sample_rate) / in_sample_rate instead of the reference's running product.
 * audio_samples aliases the demodulator's buffer.  An unknown demodulate_type has no demodulator and leaves
 * audio_samples NULL (the phase still advances).  samples_i / samples_q stay NULL and samples_length 0: nothing is
 * allocated per call (the reference reallocates both on every call). */
typedef struct {
    int in_sample_rate;
    int out_sample_rate;
    nrf_demodulate_type demodulate_type;
    void *demodulator;
    nrf_freq_shifter *freq_shifter;
    double *samples_i;
    double *samples_q;
    int samples_length;
    double *audio_samples;
    int audio_samples_length;
    void *backend; /* fsea_demod* (libfsea_hip.so) */
} nrf_decoder;

nrf_decoder *nrf_decoder_new(nrf_demodulate_type demodulate_type, int in_sample_rate, int out_sample_rate, int freq_offset);
void nrf_decoder_process(nrf_decoder *decoder, uint8_t *buffer, size_t length);
/* ADDITION: defined but not declared by the reference (src/nrf.c:1086). */
void nrf_decoder_free(nrf_decoder *decoder);

/* ---- Player (src/nrf.h:278-301, src/nrf.c:1096-1280), without an audio device ---- */

/* The decode handler (on the device's replay thread) copies device->samples under data_mutex, decodes
 * NRF_SAMPLES_LENGTH pairs and converts to (int16_t)(audio * 32000), the reference's PCM.  Each chunk is queued in a
 * bounded queue of NRF_PLAYER_QUEUE chunks (the oldest dropped when full) and, if NRF_PLAYER_PCM=<path> was set at
 * nrf_player_new, appended to that file as s16le mono at 48 kHz.  set_gain clamps to [0, 1] and stores the gain; it does
 * not scale the PCM (the reference hands unscaled PCM to OpenAL).  set_freq_offset applies from the next block.  free
 * unregisters the handler, waits for a decode in flight, and does not free the device. */
#define NRF_PLAYER_QUEUE 64

typedef struct {
    nrf_demodulate_type demodulate_type;
    nrf_device *device;
    nrf_decoder *decoder;
    float gain;              /* set_gain's clamped value */
    pthread_mutex_t mutex;   /* the queue, sequence and shutting_down */
    int shutting_down;
    int16_t *queue[NRF_PLAYER_QUEUE];
    int queue_length[NRF_PLAYER_QUEUE];
    long queue_sequence[NRF_PLAYER_QUEUE];
    int queue_head;          /* oldest chunk */
    int queue_size;
    long next_sequence;      /* decode index since nrf_player_new */
    void *pcm_file;          /* FILE* of NRF_PLAYER_PCM, or NULL */
} nrf_player;

nrf_player *nrf_player_new(nrf_device *device, nrf_demodulate_type demodulate_type, int freq_offset);
void nrf_player_set_freq_offset(nrf_player *player, int freq_offset);
void nrf_player_set_gain(nrf_player *player, float gain);
void nrf_player_free(nrf_player *player);
/* ADDITION: moves the oldest queued chunk's samples (at most `capacity`) to `out` and returns its sample count, 0 when
 * the queue is empty; *sequence (if not NULL) receives the chunk's decode index, so dropped chunks show as gaps. */
int nrf_player_pop_pcm(nrf_player *player, int16_t *out, int capacity, long *sequence);

#endif /* NRF_H */
