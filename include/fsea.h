/*
 * fsea.h -- C ABI of libfsea_hip.so: the MI355X (gfx950) IQ-FFT spectrum path.
 *
 * This is the drop-in boundary.  It sits exactly where the reference calls
 * FFTW and runs its per-sample loops on the CPU (paths under /root/reference):
 *
 *   fsea_plan_create      replaces fftw_plan_dft_1d + buffer setup
 *                         src/nrf.c:562-564, c/fft-batch.c:140-145,
 *                         c/fft-batch-broad.c:167-172
 *   fsea_exec_u8_*        replaces byte flip + unpack/centre + fftw_execute +
 *                         magnitude / dB pixel loops
 *                         src/nrf.c:100-109 (flip), 599-614 (unpack, (-1)^n),
 *                         615 (fftw_execute), 619-630 (magnitude + DC patch);
 *                         c/fft-batch.c:62-69, 83-94; c/fft-batch-broad.c:64-71,
 *                         106-121
 *   fsea_exec_f64_host    the NUT_BUFFER_F64 input branch, src/nrf.c:607-609
 *   fsea_exec_u8_shifted_* nrf_freq_shifter_process in front of the FFT, fused into its load
 *                         src/nrf.c:843-866 (shifter) + 607-612 (F64 branch);
 *                         call pattern lua/fft-shifted.lua:52-55
 *   fsea_mean_magnitude_* the 100-row "interesting?" gate,
 *                         c/fft-batch-broad.c:81-98
 *   fsea_composite_max_*  tile compositing, c/fft-stitch.c:46-54,
 *                         c/fft-stitch-broad.c:28-36
 *   fsea_plan_set_window  a taper in the weight slot of the unpack loop: the reference weights each sample by
 *                         powf(-1, ii) alone (src/nrf.c:611-612, c/fft-batch.c:65-66), i.e. its window is
 *                         rectangular; this is the optional w[n] beside it, fused into the same conversion
 *   fsea_plan_destroy     replaces fftw_destroy_plan/fftw_free
 *                         src/nrf.c:637-642, c/fft-batch.c:147-152
 *   fsea_fir_*            the IQ low-pass filter behind nrf_iq_filter: the tap design of
 *                         nrf_fir_get_low_pass_coefficients and the per-sample convolution loops of
 *                         nrf_fir_filter_get / nrf_iq_filter_get_buffer, src/nrf.c:654-775
 *   fsea_chain_*          shift -> filter -> images per block with the filtered block resident on the device
 *   fsea_zoom_*           shift -> decimating filter -> FFT: a spectrum of 1 / D of the bandwidth (nrf_decoder's chain)
 *   fsea_pfb_*            a polyphase filter bank (no counterpart in the reference): all M channels of the band at once
 *   fsea_persist_*        a persistence spectrum (no counterpart in the reference): per-bin level histograms of resident rows
 *   fsea_cfar_*           a CFAR detector across frequency (no counterpart in the reference): occupied bins, bands and masks
 *   fsea_oscfar_*         an ordered-statistic CFAR detector (no counterpart in the reference): the weaker of two close emissions
 *   fsea_tcfar_*          a CFAR detector down the time axis (no counterpart in the reference): bursts wider than a window
 *   fsea_events_*         spectrum events (no counterpart in the reference): a detection mask as runs, time-frequency boxes
 *   fsea_extract_*        event cut-outs (no counterpart in the reference): each box of fsea_events_link as decimated IQ
 *   fsea_measure_*        signal measures (no counterpart in the reference): power, offset, width and envelope of each cut-out
 *   fsea_audio_*          cut-out audio: the FM discriminator of nrf_demodulate's WBFM branch, src/nrf.c:969-993, or the AM
 *                         envelope, low-passed and decimated, for every cut-out of a table at once
 *   fsea_detect_*         the burst detector of lua/signal-detector.lua: the two loops of nrf_signal_detector_process,
 *                         src/nrf.c:883-898, as integer sums over many blocks per launch
 *   fsea_capture_*        that scene on a resident recording: detect -> gate -> filter the bursts -> line images
 *   fsea_iq_*             the IQ constellation images: the per-sample loops of nrf_buffer_to_iq_points /
 *                         nrf_device_get_iq_buffer and the Bresenham rasteriser of nrf_buffer_to_iq_lines /
 *                         nrf_device_get_iq_lines, src/nrf.c:359-421, 519-553
 *
 * Plain C: pointers, sizes and ints only; no HIP or torch types.  Device
 * pointers and streams cross the boundary as void* (a hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream).  Every function returns 0 on
 * success or a negative FSEA_E* code; fsea_last_error_string() describes the
 * last failure on the calling thread.  There is no CPU fallback: without a
 * usable gfx950 device plan creation fails with FSEA_ENODEVICE.
 */
#ifndef FSEA_H
#define FSEA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fsea_plan fsea_plan;
typedef struct fsea_history fsea_history;
typedef struct fsea_fir fsea_fir;
typedef struct fsea_iq_draw fsea_iq_draw;
typedef struct fsea_chain fsea_chain;
typedef struct fsea_zoom fsea_zoom;
typedef struct fsea_pfb fsea_pfb;
typedef struct fsea_persist fsea_persist;
typedef struct fsea_cfar fsea_cfar;
typedef struct fsea_oscfar fsea_oscfar;
typedef struct fsea_tcfar fsea_tcfar;
typedef struct fsea_events fsea_events;
typedef struct fsea_extract fsea_extract;
typedef struct fsea_demod fsea_demod;
typedef struct fsea_interp fsea_interp;
typedef struct fsea_trace fsea_trace;
typedef struct fsea_detect fsea_detect;
typedef struct fsea_capture fsea_capture;

/* Epilogue modes.  Output element type and row length are per mode. */
enum {
    /* sqrt(re^2+im^2) as f32, bin n/2 := bin n/2-1 (src/nrf.c:619-630). */
    FSEA_MODE_MAG_F32 = 0,
    /* clamp_u8(trunc(10*log10(re^2+im^2+1e-20)*10)) (c/fft-batch.c:83-94).  The f32 kernels form d = 100 log10(p) and
     * convert with v_cvt_pk_u8_f32 (round to nearest even) after lowering d by 0.5 - 2^-25: trunc(d) except for d within
     * ~8e-6 above an odd integer, where the pixel comes out one grey level low -- about one pixel in 2.5e5, inside the
     * stated pixel tolerance (exact on >= 99.9 %, +-1 elsewhere: the f32 logarithm itself moves more pixels than that
     * across an integer boundary); tests/test_emu_kernels.py::test_biased_pixel_rounding_equals_truncation_on_a_dense_sweep pins it.  The Bluestein /
     * four-step sizes truncate in a plain epilogue kernel. */
    FSEA_MODE_DB10_U8 = 1,
    /* same with *5 and pixel n/2 := pixel n/2-1 (c/fft-batch-broad.c:106-121). */
    FSEA_MODE_DB5_U8_DCFIX = 2,
    /* the complex spectrum itself, interleaved f32 re,im (what fft_out holds). */
    FSEA_MODE_COMPLEX_F32 = 3,
    /* magnitude without the DC patch. */
    FSEA_MODE_MAG_NODC_F32 = 4,
    /* 10*log10(re^2+im^2+1e-20) as f32 (log-magnitude, no quantisation). */
    FSEA_MODE_DB_F32 = 5
};

enum {
    FSEA_OK = 0,
    FSEA_EINVAL = -1,    /* bad argument (size, hop, alignment, mode) */
    FSEA_ENODEVICE = -2, /* no usable gfx950 device / HIP runtime failure at init */
    FSEA_ENOMEM = -3,
    FSEA_EHIP = -4       /* a HIP call failed; see fsea_last_error_string() */
};

/* Number of visible HIP devices (0 and FSEA_ENODEVICE when there are none). */
int fsea_device_count(int *count);

/* fft_size: powers of two from 32 to 16384 have kernels of their own (the scripts and tools of the reference use
 * 128 ... 16384).  fftw_plan_dft_1d (src/nrf.c:564) takes any size; the others run on those kernels:
 *   - powers of two from 32768 to 2^20: two passes of the kernels (four-step: n = n1 n2, column transforms, twiddle,
 *     row transforms) and three helper kernels;
 *   - everything else from 2 to 2^19: Bluestein's algorithm, two transforms of size 2^p >= 2 fft_size - 1 around a
 *     pointwise product with the chirp's spectrum.
 * Same modes, same tolerance.  Such a plan serves fsea_exec_u8_device, the three *_host entry points, the history ring
 * and the gate, but not the tiled and the frequency-shifted entry points (FSEA_EINVAL); it is a compatibility path, not
 * a tuned one: five to ten launches per batch through work buffers that belong to the plan, so launches of one such plan
 * on different streams run one after the other (ordered by events), and they cannot be captured into a graph.
 * Larger sizes fail with FSEA_EINVAL.
 * hop: samples between successive frame starts (hop == fft_size: back-to-back
 * frames as in c/fft-batch.c; hop < fft_size: overlapped STFT).  hop must be a
 * positive multiple of 8 for the sizes with kernels of their own, any positive number for the others.
 * device: HIP device ordinal. */
int fsea_plan_create(fsea_plan **plan, int fft_size, int hop, int mode, int device);
int fsea_plan_destroy(fsea_plan *plan);

/* Taper window.  With a window set, every u8 transform of the plan computes
 *   X[k] = sum_n (-1)^n w[n] (u8[n] / 256) e^{-2 pi i n k / fft_size}
 * -- the reference's unpack loop (src/nrf.c:601-614) with w[n] beside its powf(-1, ii); w == 1 is the reference
 * itself -- followed by the plan's epilogue unchanged (MAG and DB5 rows still copy bin n/2 - 1 into bin n/2: with a
 * taper the offset-binary DC term also reaches the neighbours of bin n/2, as it does in the reference's arithmetic).
 * The multiply is fused into the kernel's byte conversion (one packed multiply per sample; no extra pass, no extra
 * HBM traffic: the fft_size weights live in L2 / registers).
 *   w: fft_size floats, copied; NULL removes the window (rectangular, the un-windowed kernels).  Any finite values.
 * Applies to every transform of the plan: fsea_exec_u8_device, fsea_exec_u8_tiled_device, fsea_exec_u8_host, the history
 * ring, the gate, and -- since round 5 -- the frequency-shifted entry points (fsea_exec_u8_shifted_*: x[n] = (-1)^n w[n]
 * ((u8/256) e^{i phi} + 0.5 (1 + i)), kernels `*_u8_rot_win`) and the f64-input one (fsea_exec_f64_host: x[n] = (-1)^n
 * w[n] f64[n], src/nrf.c:607-612 with the taper beside the sign, kernels `*_f32_win`), i.e. the whole
 * nrf_freq_shifter -> nrf_fft chain of lua/fft-shifted.lua:52-55.  fsea_plan_set_window fails with FSEA_EINVAL on a plan
 * whose size has no kernel of its own (not a power of two in [32, 16384]).  fsea_plan_kernel_name's pointer stays valid
 * across this call (both names live as long as the plan); what it points to is the name in use when it was asked.
 * Synchronous (waits for the device); not to be called while another thread is launching the plan.
 * Precision: the kernels transform w[n] (u8[n] - 128) and add the offset-binary DC term back as its known spectrum
 * (computed in double at this call) when that spectrum is confined to the bins around n/2 -- every cosine-sum
 * taper (Hann, Hamming, Blackman, Blackman-Harris, flat-top; fsea_plan_window_form() == 1; what is left out is the
 * f32 rounding of the weights themselves, ~2e-8 of the DC term's rms).  Any other w (Kaiser, a truncated Gaussian,
 * arbitrary values) is applied to the offset-binary values themselves (form 2): same result, f32 rounding noise
 * relative to the DC term instead of to the signal (~1.2e-7 of the DC term's rms in every bin; inside the stated
 * tolerance either way). */
int fsea_plan_set_window(fsea_plan *plan, const float *w);
/* 0 = no window, 1 = centred form, 2 = offset-binary form (see above). */
int fsea_plan_window_form(const fsea_plan *plan);

/* Standard tapers in their periodic ("DFT-even") form, w[j] = sum_k (-1)^k a_k cos(2 pi k j / n) -- what
 * scipy.signal.get_window(name, n) returns -- evaluated in double, rounded to float. */
enum {
    FSEA_WINDOW_RECT = 0,
    FSEA_WINDOW_HANN = 1,            /* 0.5, 0.5 */
    FSEA_WINDOW_HAMMING = 2,         /* 0.54, 0.46 */
    FSEA_WINDOW_BLACKMAN = 3,        /* 0.42, 0.5, 0.08 */
    FSEA_WINDOW_BLACKMANHARRIS = 4,  /* 0.35875, 0.48829, 0.14128, 0.01168 */
    FSEA_WINDOW_FLATTOP = 5          /* 0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368 */
};
int fsea_window_fill(int kind, int n, float *w);

/* Launch geometry the plan would use for n_frames (persistent grid, workgroup
 * size, static LDS bytes per workgroup).  Any out-pointer may be NULL. */
int fsea_plan_grid(const fsea_plan *plan, size_t n_frames, unsigned *grid, unsigned *block,
                   size_t *lds_bytes);

/* Bytes of one output row for the plan's mode (fft_size * element size). */
size_t fsea_plan_row_bytes(const fsea_plan *plan);
int fsea_plan_fft_size(const fsea_plan *plan);

/* How a launch's frames are handed to the persistent workgroups of the sizes whose frames span several wavefronts
 * (4096 points and up): FSEA_UNITS_TICKETS = atomic ticket pools per XCD with stealing (evens out unequal progress;
 * best from more than 16 units -- frames, pairs of frames at 4096 points -- per workgroup, which is where AUTO
 * switches), FSEA_UNITS_STATIC = unit k of workgroup b is b + k * grid (no atomics;
 * best for short launches), FSEA_UNITS_AUTO (default) = chosen per launch by its length.  Results are identical; the
 * setting exists for measurements and tests.  Takes effect from the next launch; not to be changed while another
 * thread is launching the plan. */
#define FSEA_UNITS_AUTO 0
#define FSEA_UNITS_STATIC 1
#define FSEA_UNITS_TICKETS 2
int fsea_plan_set_unit_distribution(fsea_plan *plan, int policy);

/* Device-resident execution.  d_iq: device pointer to interleaved 8-bit IQ,
 * at least 2*((n_frames-1)*hop + fft_size) bytes, 16-byte aligned.
 * flip != 0: bytes are raw HackRF int8 and the kernel applies b ^ 0x80
 * (src/nrf.c:103-106); flip == 0: bytes are already offset-binary (RTL-SDR).
 * d_out: device pointer, n_frames rows of fsea_plan_row_bytes().
 * stream: hipStream_t as void*; NULL is HIP's null (default) stream, which is
 * also what torch.cuda.current_stream().cuda_stream is unless a side stream
 * is current.  Asynchronous with respect to the host.
 * A plan may be launched from several host threads and on any number of streams; launches on
 * one stream run in order, launches on different streams may overlap (up to 64 long launches in flight at a time;
 * a 65th waits for the oldest -- inside the call, holding the plan's slot table, so that other threads launching
 * the same plan wait with it).  The calls leave the caller's current HIP device unchanged.
 * The call enqueues one kernel; a long launch of the multi-wave sizes (4096 points and up, frames handed out by the
 * ticket pools) additionally records an event behind it, by which its counter slot is recycled.  While the stream is
 * being captured into a hipGraph nothing but the kernel is enqueued
 * (launch-bound consumers: tests/test_gpu_parity.py::test_launches_can_be_captured_into_a_hip_graph); a captured
 * launch keeps the ticket-counter slot of the stream it was captured on: replay one instance of such a graph at a
 * time, on the stream it was captured on or in order with that stream's other launches of the plan.  The slot stays
 * reserved for that stream until fsea_plan_reset (the graph's kernel node holds its address; the stream's own un-captured
 * launches go on using it): at most 64 distinct streams may hold captured launches of one plan at a time
 * (fsea_plan_release_stream gives one stream's slot back once its graphs are destroyed; fsea_plan_reset releases them all
 * and invalidates the graphs).  Plans of the sizes without a
 * kernel of their own (Bluestein / four-step) refuse a capturing stream with FSEA_EINVAL. */
int fsea_exec_u8_device(fsea_plan *plan, const void *d_iq, size_t n_frames, int flip,
                        void *d_out, void *stream);

/* The same transform with the rows written straight into a stitched image: the launch's frames are
 * consecutive `tile_rows`-row tiles (frame f = row f % tile_rows of tile f / tile_rows), and tile k lands
 * at columns [first_x + k*tile_step, ... + fft_size) of rows 0..tile_rows-1 of d_image (image_rows rows of
 * image_stride elements of the plan's output type).  Tiles are WRITTEN, not max-composited, so tile_step
 * must be >= fft_size; on a zeroed image that equals img_gray_copy's max() of c/fft-stitch-broad.c:62-87
 * (WIDTH_STEP == FFT_SIZE there), without the tile stack, the image read and the second pass.  Overlapping
 * tiles (c/fft-stitch.c, step < fft_size) go through fsea_exec_u8_device + fsea_stitch_tiles_device.
 * n_frames must be whole tiles; tile_rows a multiple of the size's frames per workgroup (1 for
 * fft_size >= 8192, 2 at 4096, ... 64 at 32: powers of two up to 64 always work); image_stride, first_x,
 * tile_step multiples of 4 elements; d_image 16-byte aligned. */
int fsea_exec_u8_tiled_device(fsea_plan *plan, const void *d_iq, size_t n_frames, int flip, void *d_image,
                              size_t image_rows, size_t image_stride, size_t first_x, size_t tile_rows,
                              size_t tile_step, void *stream);

/* Host-buffer execution; returns when `out` is complete.  Batches of up to 256 KiB (in + out: one nrf_fft_process
 * row) run as ONE launch on device-mapped pinned staging.  Larger ones are pipelined in chunks of whole frames: chunk
 * c travels to the device while chunk c-1 is transformed and the rows of chunk c-2 travel back, on three streams --
 * the streaming shape of the reference's tools (c/fft-batch.c:54-102: a transfer in, a row out) at the granularity a
 * PCIe link wants.  `iq` and `out` may be any host memory; pages that are not pinned yet are pinned in place for the
 * duration of the call (hipHostRegister) so that the two directions overlap, and memory from fsea_host_alloc (or
 * hipHostMalloc) skips that step.  Link-bound: 64 MiB in + 128 MiB out in 2.6-2.9 ms on an MI355X host
 * (profiles/r03_host_path.txt).  The same holds for the _shifted_ and _f64_ forms below. */
int fsea_exec_u8_host(fsea_plan *plan, const uint8_t *iq, size_t n_frames, int flip,
                      void *out);

/* Frequency-shifted spectrum, the device-resident form of
 *   nrf_freq_shifter_process(shifter, samples); nrf_fft_process(fft, shifter_buffer)
 * (src/nrf.c:843-866, 598-631; lua/fft-shifted.lua:52-55) with the rotation fused into the FFT
 * kernel's load.  Stream sample m (frame f, sample n: m = f*hop + n) becomes
 *   y[m] = (u8[m] / 256) * e^{+2 pi i (phase0_cycles + m * cycles_per_sample)} + 0.5 (1 + i)
 * and frame f transforms x[n] = (-1)^n y[f*hop + n]; epilogue per the plan's mode.
 * cycles_per_sample = freq_offset / sample_rate; phase0_cycles continues a stream across calls
 * (a shifter that has consumed M samples is at phase M * cycles_per_sample).  Other arguments
 * as fsea_exec_u8_device / fsea_exec_u8_host. */
int fsea_exec_u8_shifted_device(fsea_plan *plan, const void *d_iq, size_t n_frames, int flip,
                                double cycles_per_sample, double phase0_cycles, void *d_out,
                                void *stream);
int fsea_exec_u8_shifted_host(fsea_plan *plan, const uint8_t *iq, size_t n_frames, int flip,
                              double cycles_per_sample, double phase0_cycles, void *out);

/* F64 interleaved complex input (src/nrf.c:607-609: no /256, no flip). */
int fsea_exec_f64_host(fsea_plan *plan, const double *iq, size_t n_frames, void *out);

/* Device-resident history of MAG_F32 rows, newest first: nrf_fft's `buffer` (src/nrf.h:133,
 * src/nrf.c:565, 616-617) kept in HBM as a ring.  push = one nrf_fft_process: the kernel writes the
 * new row straight into the ring (the reference memmoves the whole history by one row first);
 * shift = nrf_fft_shift's per-row scroll for an integer number of bins (src/nrf.c:569-596: > 0 moves
 * rows left, < 0 right, vacated bins zero, |shift| >= fft_size clears the history), as a kernel;
 * get = nrf_fft_get_buffer: ONE device-to-host transfer of rows * fft_size f32 and one widening to
 * f64 into `out` (rows * fft_size doubles).  The plan must be a MAG_F32 plan and must outlive every
 * push / shift / get on the history (destroy the history first; fsea_history_destroy itself no longer touches the
 * plan).  All calls are synchronous. */
int fsea_history_create(fsea_plan *plan, int rows, fsea_history **history);
int fsea_history_destroy(fsea_history *history);
int fsea_history_push_u8_host(fsea_history *history, const uint8_t *iq, int flip);
int fsea_history_push_f64_host(fsea_history *history, const double *iq);
int fsea_history_shift(fsea_history *history, int shift);
int fsea_history_get_f64(fsea_history *history, double *out);

/* Mean of sqrt(re^2+im^2) over the first n_frames rows of a device-resident
 * u8 IQ block (c/fft-batch-broad.c:81-98).  Synchronous. */
int fsea_mean_magnitude_u8_device(fsea_plan *plan, const void *d_iq, size_t n_frames,
                                  int flip, double *mean, void *stream);

/* dst[dst_y + y][dst_x + j] = max(dst, src[y][j]) for a width x height u8 tile
 * (c/fft-stitch.c:46-54).  dst is dst_height rows of dst_stride pixels; a tile that does not lie
 * inside it is rejected with FSEA_EINVAL (nothing is written).  Device pointers; asynchronous on
 * `stream`. */
int fsea_composite_max_device(void *d_dst, const void *d_src, uint32_t dst_x,
                              uint32_t dst_y, uint32_t width, uint32_t height,
                              uint32_t dst_stride, uint32_t dst_height, uint32_t src_stride, int device,
                              void *stream);

/* The whole stitch loop of c/fft-stitch*.c:167-189 for a contiguous stack of tiles
 * ([k][y][x], each width x height): tile k is max-composited at x = first_x +
 * k * width_step.  Overlapping neighbours (width_step < width) are processed in
 * separate race-free launches.  Device pointers; asynchronous on `stream`. */
int fsea_stitch_tiles_device(void *d_image, const void *d_tiles, uint32_t n_tiles, uint32_t first_x,
                             uint32_t width_step, uint32_t width, uint32_t height,
                             uint32_t image_stride, int device, void *stream);

/* Pinned (page-locked) host memory for the buffers handed to the *_host entry points, so that C callers need no HIP
 * headers: copies from and to it are asynchronous without a per-call registration.  Free with fsea_host_free. */
int fsea_host_alloc(size_t bytes, void **ptr);
int fsea_host_free(void *ptr);

/* Small device-memory helpers so that C callers need no HIP headers. */
int fsea_device_alloc(int device, size_t bytes, void **d_ptr);
int fsea_device_free(int device, void *d_ptr);
int fsea_copy_to_device(int device, void *d_dst, const void *src, size_t bytes);
int fsea_copy_to_host(int device, void *dst, const void *d_src, size_t bytes);
/* Waits for `stream` (NULL = the null stream) on the plan's device. */
int fsea_stream_synchronize(fsea_plan *plan, void *stream);

/* Streams and asynchronous copies for C callers (a hipStream_t as void*, non-blocking with respect to the null stream).
 * A consumer of independent batches -- captures of a sweep, blocks of a stream -- submits consecutive batches
 * ALTERNATELY ON TWO STREAMS with double-buffered device memory: upload, transform and download of batch k + 1 overlap
 * the drain of batch k, and the ramp and tail of each launch (a few microseconds in which the chip is not full) are
 * covered by its neighbour: +8...12 % on resident batches (bench.py: extra.two_stream_*), more when copies are in the
 * loop.  INTEGRATION.md section 2 shows the pattern; fsea-fft-batch and fsea-fft-sweep use it.  Host memory should come
 * from fsea_host_alloc (pinned), or the copies fall back to staged, synchronous ones. */
int fsea_stream_create(int device, void **stream);
int fsea_stream_destroy(int device, void *stream);
int fsea_copy_to_device_async(int device, void *d_dst, const void *src, size_t bytes, void *stream);
int fsea_copy_to_host_async(int device, void *dst, const void *d_src, size_t bytes, void *stream);

/* Recovery after an aborted launch (device fault, killed context): waits for the device and
 * re-zeroes the plan's internal frame-distribution counters.  Not needed in normal operation. */
int fsea_plan_reset(fsea_plan *plan);

/* Gives back the frame-distribution counter slot `stream` holds in this plan, in particular one reserved by a captured
 * launch: call it once the hipGraphs captured on that stream are destroyed (before destroying the stream), so that an
 * application capturing on short-lived streams does not run out of the 64 slots.  Waits for the stream's last un-captured
 * launch of the plan.  FSEA_OK also when the stream holds no slot; FSEA_EINVAL while the stream is capturing. */
int fsea_plan_release_stream(fsea_plan *plan, void *stream);

/* Name of the kernel the plan launches for raw int8 input (flip != 0), for matching rocprof rows:
 * MAG_F32, DB5_U8_DCFIX and DB10_U8 plans have compile-time kernels (`*_u8_mag`, `*_u8_db5`,
 * `*_u8_db10`); the other modes, and any mode with flip == 0, run the run-time-mode kernel `*_u8`.
 * Kernel variants, per-workgroup traces and the timing helper live in the separate tuning
 * library (include/fsea_tune.h, libfsea_hip_tune.so); this library has one kernel set per size. */
const char *fsea_plan_kernel_name(const fsea_plan *plan);

/* Streaming complex FIR filter with real taps: the IQ low-pass filter of the reference (src/nrf.c:654-775), one kernel
 * launch per call.  Output i of a call on n samples x is
 *   y[i] = sum_{k < L} c[k] x_ext[i + k],   x_ext = tail ++ x,  i < n,
 * where the tail holds the last L - 1 samples of the previous calls (zeros after create and reset); after the call the
 * tail is the last L - 1 values of x_ext (also when n < L - 1).  I and Q are filtered independently by the same taps.
 * f32 taps, f32 arithmetic (one packed FMA per output sample and tap); output interleaved f32 (I, Q).
 * Inputs: interleaved 8-bit IQ read as u8 / 256 (flip != 0: raw HackRF int8 bytes, b ^ 0x80 first, as
 * fsea_exec_u8_device), or interleaved f64 IQ read as is (narrowed to f32). */
#define FSEA_FIR_MAX_TAPS 512

/* The reference's window-method low-pass design (nrf_fir_get_low_pass_coefficients, src/nrf.c:654-676) in double,
 * bit for bit: m = length + (length + 1) % 2 taps are designed and normalised to sum 1, and the first `length` of them are
 * written to taps -- for an even length that is the reference's filter as nrf_fir_filter_new uses it (asymmetric, not
 * summing to 1).  Host arithmetic; needs no device. */
int fsea_fir_lowpass_taps(double sample_rate, double half_ampl_freq, int length, double *taps);

/* n_taps in [1, FSEA_FIR_MAX_TAPS]; the taps are copied (rounded to f32).  FSEA_EINVAL for a NULL pointer, n_taps out of
 * range or a non-finite tap (checked before any device work); FSEA_ENODEVICE without a GPU.  Destroy waits for the device. */
int fsea_fir_create(fsea_fir **fir, const double *taps, int n_taps, int device);
int fsea_fir_destroy(fsea_fir *fir);
/* Zeroes the tail (a fresh object's state).  Synchronous: waits for the device first. */
int fsea_fir_reset(fsea_fir *fir);
int fsea_fir_n_taps(const fsea_fir *fir);

/* Device-resident form: d_iq holds 2 * n_samples bytes, d_out receives n_samples (I, Q) float pairs; both 16-byte aligned.
 * Asynchronous on `stream`.  Calls on one object take effect in stream order: successive calls on one stream continue one
 * signal; across streams the caller orders them (the tail of call k is read by call k + 1). */
int fsea_fir_u8_device(fsea_fir *fir, const void *d_iq, size_t n_samples, int flip, void *d_out, void *stream);
/* Host-buffer forms; return when `out` (2 * n_samples floats) is complete.  Staged through pinned memory on the object's
 * own stream; calls on one object from several threads are serialised. */
int fsea_fir_u8_host(fsea_fir *fir, const uint8_t *iq, size_t n_samples, int flip, float *out);
int fsea_fir_f64_host(fsea_fir *fir, const double *iq, size_t n_samples, float *out);

/* The filter with nrf_freq_shifter_process (src/nrf.c:843-866) fused into its load: kernel fsea_shift_fir_u8.  Sample m of
 * the call stands at position P = sample_offset + m of the stream and becomes
 *   x[m] = (u8[m] / 256) * e^{+2 pi i (phase0_cycles + P * cycles_per_sample)} + 0.5 (1 + i)
 * (the offset-binary value itself is rotated, then 0.5 is added to both parts), and the filter runs on tail ++ x as above;
 * the tail holds rotated samples.  cycles_per_sample = freq_offset / sample_rate.
 * Continuing a stream: keep cycles_per_sample and phase0_cycles as they are and pass the number of samples the earlier
 * calls consumed as sample_offset (0 for the first call) -- do NOT add m * cycles_per_sample into phase0_cycles, the sum
 * would round differently from call to call.  The phasor of a sample is a function of (cycles_per_sample, phase0_cycles, P)
 * alone: P * cycles_per_sample is formed as an exact two-term product, reduced modulo 1 together with phase0_cycles in
 * double and only then evaluated in float.  The reduced phase is within about 2^-50 cycles of the exact one while
 * |cycles_per_sample * P| < 2^53 (every P at |cycles_per_sample| <= 0.5); at the limits of the domain (|cycles_per_sample|
 * near 2^20, P near 2^52) it is no worse than 2^-35 cycles, 2^-36 measured -- still a thousandth of the 2^-25 the float
 * conversion rounds to (tests/test_shift_ref_host.py holds it to 2^-30 over the whole domain).  So a stream cut into calls
 * of any lengths gives the one-call result bit for bit, as for the unshifted forms.
 * FSEA_EINVAL (before any device work) for a NULL pointer, a misaligned device buffer, a non-finite phase0_cycles, a
 * cycles_per_sample that is not finite or beyond +-2^20, or sample_offset + n_samples > 2^52 (the last sample may stand at
 * position 2^52 - 1).  Other arguments as fsea_fir_u8_device / fsea_fir_u8_host. */
int fsea_fir_u8_shifted_device(fsea_fir *fir, const void *d_iq, size_t n_samples, int flip, double cycles_per_sample,
                               double phase0_cycles, uint64_t sample_offset, void *d_out, void *stream);
int fsea_fir_u8_shifted_host(fsea_fir *fir, const uint8_t *iq, size_t n_samples, int flip, double cycles_per_sample,
                             double phase0_cycles, uint64_t sample_offset, float *out);

/* IQ constellation images (src/nrf.c:359-421, 519-553).  The input is interleaved (I, Q) pairs of one element type:
 * FSEA_IQ_U8 bytes used as they are (flip != 0: raw HackRF int8 bytes, b ^ 0x80 first, as fsea_fir_u8_device), or
 * FSEA_IQ_F32 / FSEA_IQ_F64 values v whose coordinate is the reference's nut_buffer_get_u8 on x86-64:
 * (uint8_t)(v * 256.0) computed as cvttsd2si -- truncation to int32, 0x80000000 for NaN and anything whose truncation lies
 * outside the int32 range -- then the low byte (so -0.01 -> 254, 1.0 -> 0, NaN -> 0).  An f32 value gives the
 * coordinate of its exact f64 widening.
 *   points: a 256 x 256 u8 image, bin I * 256 + Q (I is the row), each pair adds 1 modulo 256 (the reference's u8++ wraps).
 *   lines:  a (256 m)^2 u8 image, m = size_multiplier in [1, FSEA_IQ_MAX_MULTIPLIER]; for consecutive points P[k-1], P[k]
 *           (0 < k < n_points) the reference's draw_line -- Bresenham with err = (dx > dy ? dx : -dy) / 2, both endpoints
 *           included -- adds 1 to every pixel from (I[k-1] m, Q[k-1] m) to (I[k] m, Q[k] m); pixel (x, y) is at
 *           y * 256 m + x, transposed relative to the points image.  Each pixel is min(count, 255) (pixel_inc saturates).
 * The order of the increments does not change either image: both are exact and deterministic.
 * Batched device forms: frame f is the n pairs (points) or n_points points (lines) at pair f * n of d_iq, and its image
 * is the f-th 65536-byte (points) or (256 m)^2-byte (lines) image of d_image; d_iq and d_image 16-byte aligned.
 * Asynchronous on `stream`.  The line images are counted in a u32 buffer that the object owns: its calls on several
 * streams follow one another on the device (each waits for an event the previous one recorded).
 * Host forms: one frame; return when `image` is complete; staged through pinned memory on the object's own stream, calls
 * on one object from several threads are serialised.
 * Every form checks its arguments before any device work: FSEA_EINVAL for a NULL object or buffer, an unknown type, an m
 * outside [1, FSEA_IQ_MAX_MULTIPLIER], n_frames < 0, or more than 2^31 pairs per frame.  Create: FSEA_ENODEVICE without a
 * GPU.  Destroy waits for the device. */
enum { FSEA_IQ_U8 = 0, FSEA_IQ_F32 = 1, FSEA_IQ_F64 = 2 };
#define FSEA_IQ_MAX_MULTIPLIER 16

int fsea_iq_draw_create(fsea_iq_draw **draw, int device);
int fsea_iq_draw_destroy(fsea_iq_draw *draw);
int fsea_iq_points_device(fsea_iq_draw *draw, const void *d_iq, int type, int flip, size_t n_pairs, int n_frames,
                          void *d_image, void *stream);
int fsea_iq_lines_device(fsea_iq_draw *draw, const void *d_iq, int type, int flip, size_t n_points, int n_frames,
                         int size_multiplier, void *d_image, void *stream);
int fsea_iq_points_host(fsea_iq_draw *draw, const void *iq, int type, int flip, size_t n_pairs, uint8_t *image);
int fsea_iq_lines_host(fsea_iq_draw *draw, const void *iq, int type, int flip, size_t n_points, int size_multiplier,
                       uint8_t *image);

/* The chain the reference's IQ scenes run per block (lua/dvbt.lua:46-51, lua/iq-tex-filtered.lua:44-47): optional frequency
 * shift -> low-pass filter -> constellation images, with the filtered block resident on the device between the steps.
 * The object owns a filter (fsea_fir: the stream's tail is carried from run to run), a draw object (fsea_iq_draw), the
 * device buffer of the filtered f32 pairs and pinned staging.  Nothing here computes: the kernels are those of
 * fsea_fir_u8_device / fsea_fir_u8_shifted_device and fsea_iq_points_device / fsea_iq_lines_device (FSEA_IQ_F32), so every
 * output is what those calls give, bit for bit.
 *   stage (NULL: no flip, no shift): how the bytes enter the filter.  shift != 0: rotated as fsea_fir_u8_shifted_device
 *       does, and n_zero samples of plain 0.0 follow each block through the filter in the same launch -- nrf_freq_shifter's
 *       buffer has twice the pairs of its input, the back half zero (src/nrf.c:851), and nrf_iq_filter follows its length.
 *       A frame of the result has n_samples + n_zero pairs.  n_zero needs shift != 0.
 *   outputs (NULL: none): any of a points image (65536 bytes), a lines image ((256 m)^2 bytes, the first n_line_points
 *       pairs of the frame joined, n_line_points <= its pairs) and the f32 pairs themselves, per frame.
 *   run_host:   one block of n_samples 8-bit pairs from host memory (2 n_samples bytes up), the outputs into host memory;
 *               one stream, one synchronisation at the end.  run_f64_host: the same for f64 pairs (no flip, no shift).
 *   fetch_host: more outputs of the resident block of the last host run (another m or n_line_points), nothing uploaded.
 *   run_device: n_frames consecutive blocks of one stream behind d_iq -> n_frames images and frames of pairs in device
 *               memory, asynchronous on `stream`; the same bytes as n_frames single runs.  Without zero samples it is one
 *               filter launch; with them one per block, which then needs n_samples a multiple of 8 and n_zero even
 *               (16-byte-aligned pieces).  The filtered pairs pass through the object's buffer: runs on several streams
 *               are the caller's to order.  d_iq and every output 16-byte aligned.
 * Every form checks its arguments before any device work and before it looks into the object (FSEA_EINVAL as the calls it
 * is made of; more than 2^31 pairs per frame).  With shift != 0 that includes the limits of fsea_fir_u8_shifted_* for the
 * whole call: frame f stands at sample_offset + f * n_samples -- the n_zero samples are no samples of the stream and do not
 * count -- so sample_offset + n_frames * n_samples <= 2^52.  With shift == 0 cycles_per_sample, phase0_cycles and
 * sample_offset are not looked at.  A refused call changes nothing: the resident block, fsea_chain_n_pairs, the filter's
 * tail and the caller's outputs are as before it.  Create: as fsea_fir_create, FSEA_ENODEVICE without a GPU.  Destroy and reset (a zero tail) wait for the device.
 * Calls on one object from several threads are serialised. */
typedef struct {
    int flip;                 /* != 0: raw HackRF int8 bytes */
    int shift;                /* != 0: frequency shift in front of the filter */
    double cycles_per_sample; /* as fsea_fir_u8_shifted_device; sample_offset is the position of the call's first sample */
    double phase0_cycles;
    uint64_t sample_offset;
    size_t n_zero;            /* zero samples behind each block (shift != 0 only) */
} fsea_chain_stage;

typedef struct {
    void *points;             /* NULL, or 65536 bytes per frame */
    void *lines;              /* NULL, or (256 size_multiplier)^2 bytes per frame */
    int size_multiplier;      /* of the lines image, in [1, FSEA_IQ_MAX_MULTIPLIER] */
    size_t n_line_points;
    void *pairs;              /* NULL, or 2 (n_samples + n_zero) floats per frame */
} fsea_chain_outputs;

int fsea_chain_create(fsea_chain **chain, const double *taps, int n_taps, int device);
int fsea_chain_destroy(fsea_chain *chain);
int fsea_chain_reset(fsea_chain *chain);
/* pairs per frame of the resident block (0 before the first run) */
size_t fsea_chain_n_pairs(const fsea_chain *chain);
int fsea_chain_run_host(fsea_chain *chain, const uint8_t *iq, size_t n_samples, const fsea_chain_stage *stage,
                        const fsea_chain_outputs *outputs);
int fsea_chain_run_f64_host(fsea_chain *chain, const double *iq, size_t n_samples, const fsea_chain_outputs *outputs);
int fsea_chain_fetch_host(fsea_chain *chain, const fsea_chain_outputs *outputs);
int fsea_chain_run_device(fsea_chain *chain, const void *d_iq, size_t n_samples, int n_frames, const fsea_chain_stage *stage,
                          const fsea_chain_outputs *d_outputs, void *stream);

/* The zoom spectrum: frequency shift -> low-pass -> keep every D-th sample -> FFT, the chain the reference runs inside
 * nrf_decoder (nrf_freq_shifter, nrf_downsampler at rate_mul = D, nrf_fft) as one object.  A call hands in n_samples
 * interleaved 8-bit IQ samples at stream position sample_offset.  With x the rotated samples of fsea_fir_u8_shifted_*
 * above (same flip, cycles_per_sample, phase0_cycles and sample_offset; no zero half) and x_ext = tail ++ x,
 *   pairs[i] = sum_{k < L} c[k] x_ext[i D + k],   i < n_out = n_samples / D (rounded down),
 * and afterwards the tail is the last L - 1 values of x_ext (also when n_samples < L - 1, and when n_samples < D: no
 * output, the tail still advances).  Kernel fsea_shift_decim_u8: the staging arithmetic of fsea_shift_fir_u8, one FMA chain
 * per output with the taps ascending, so pairs[i] is output i D of fsea_fir_u8_shifted_device with the same taps, state and
 * arguments, bit for bit; a stream cut into calls at multiples of D gives the one-call result bit for bit.  The decimation
 * phase restarts with every call (the reference's nrf_downsampler_process restarts t = 0 per block): a call whose length is
 * not a multiple of D drops its last n_samples mod D samples from the decimated sequence (they still enter the tail), and
 * the next call's output 0 stands at its own sample 0.
 * The object owns an ordinary plan (fft_size, hop, mode; hop counted in decimated samples) and the device buffer of the
 * pairs.  Behind the decimating launch the plan transforms the pairs on the same stream: row r covers the decimated
 * samples [r hop, r hop + fft_size) of THIS call, n_out >= fft_size ? (n_out - fft_size) / hop + 1 : 0 rows.  Decimated
 * samples that do not fill a row are not carried to the next call; the filter's tail is, and the stream position is the
 * caller's sample_offset.  The rows are those of fsea_exec_f64_host of such a plan on the pairs, bit for bit.
 *   create:     decimation in [1, FSEA_ZOOM_MAX_DECIMATION], n_taps in [1, FSEA_FIR_MAX_TAPS] (the taps are copied, rounded to
 *               f32); fft_size, hop and mode as fsea_plan_create, with its statuses.  FSEA_EINVAL for a NULL pointer, n_taps or
 *               decimation out of range or a non-finite tap, checked before any device work; FSEA_ENODEVICE without a GPU.
 *   reset:      a zero tail; synchronous.  set_window: fsea_plan_set_window of the inner plan.
 *   run_device: d_iq (2 n_samples bytes), d_rows (out_rows x row_bytes) and d_pairs (NULL, or 2 n_out floats), 16-byte
 *               aligned; asynchronous on `stream`.  The pairs pass through the object's buffer: a call on any stream waits for
 *               the previous call of the object (an event), so successive calls continue one signal.
 *   run_host:   the same from and to host memory through pinned staging on the object's own stream; returns when rows and
 *               pairs are complete.  Calls on one object from several threads are serialised.
 * Both check before any device work: FSEA_EINVAL for a NULL object or buffer (d_rows / rows only where the call yields a row),
 * a misaligned device buffer, more than 2^31 samples, and the cycles_per_sample, phase0_cycles and sample_offset limits of
 * fsea_fir_u8_shifted_*.  Destroy waits for the device. */
#define FSEA_ZOOM_MAX_DECIMATION 64
#define FSEA_ZOOM_TILE_OUTPUTS 128   /* outputs per workgroup of fsea_shift_decim_u8 */
int fsea_zoom_create(fsea_zoom **zoom, const double *taps, int n_taps, int decimation, int fft_size, int hop, int mode,
                     int device);
int fsea_zoom_destroy(fsea_zoom *zoom);
int fsea_zoom_reset(fsea_zoom *zoom);
int fsea_zoom_set_window(fsea_zoom *zoom, const float *w);
size_t fsea_zoom_out_pairs(const fsea_zoom *zoom, size_t n_samples);
size_t fsea_zoom_out_rows(const fsea_zoom *zoom, size_t n_samples);
size_t fsea_zoom_row_bytes(const fsea_zoom *zoom);
int fsea_zoom_run_device(fsea_zoom *zoom, const void *d_iq, size_t n_samples, int flip, double cycles_per_sample,
                         double phase0_cycles, uint64_t sample_offset, void *d_rows, void *d_pairs, void *stream);
int fsea_zoom_run_host(fsea_zoom *zoom, const uint8_t *iq, size_t n_samples, int flip, double cycles_per_sample,
                       double phase0_cycles, uint64_t sample_offset, void *rows, float *pairs);

/* The polyphase filter bank: the whole band split into M channels, every D-th output of each, D = M / q.  A prototype
 * low-pass c of L = M P taps (doubles, copied as f32) is folded into M branches of P taps; one M-point transform of the
 * object's own plan follows per frame.  State between calls: the tail (the last L - 1 samples of earlier calls, zero after
 * create and reset) and s0, the samples earlier calls consumed since create or reset.  A call reads its n_samples 8-bit
 * pairs as the other u8 entry points do (u8 / 256; flip != 0: b ^ 0x80 first).  With x_ext = tail ++ x and
 * F = n_samples / D (rounded down), for t < F and r < M
 *   v_t[r] = sum_{p < P} c[p M + r] x_ext[t D + p M + r]       one f32 FMA chain per output, p ascending, from +0
 *   frames[t][(r + s0 + t D) mod M] = v_t[r]
 *   rows[t] = the plan (size M, hop M, the object's mode) on frames[t] as f32 input,
 * which, M being even, is with the plan's (-1)^m centring
 *   X_t[k] = sum_{j < L} c[j] x_ext[t D + j] e^{-2 pi i (k - M/2)(s0 + t D + j) / M}:
 * column k of a row is the band centred at (k - M/2) rate / M, mixed to zero with a phase tied to the stream position,
 * filtered by c, every D-th output.  Column M/2 is the centre channel and carries the offset-binary DC term; MAG and DB5
 * rows get the plan's usual DC patch there.  Afterwards the tail is the last L - 1 values of x_ext (also when
 * n_samples < L - 1) and s0 += n_samples: a stream cut at multiples of D gives the one-call result bit for bit; the
 * n_samples mod D samples a call leaves over stay in the tail, and the next call's frames start at its own sample 0 (the
 * zoom's convention).  v_t[r] is output t D of fsea_fir_u8_device with the taps c[p M + r] at p M + r and zeros elsewhere,
 * as a value; the rows are those of fsea_exec_f64_host of such a plan on the frames, bit for bit.
 * Kernel fsea_pfb_frames_u8: a workgroup of 256 lanes owns T frames x C columns and stages T + (2 ceil(P / 2) - 1) q rows
 * of C samples in LDS: the smallest image of 20, 40 and 80 KiB, and in it the widest C of min(M, 256), 128 and 64, that
 * leave T >= twice those extra rows (64 columns in 80 KiB where none does), T <= 128 a multiple of the 256 / C frames
 * the lanes work on at a time.  Kernel fsea_pfb_transpose:
 * series[k F + t] = rows[t][k], the F outputs of channel k in a row.
 *   prototype:  host arithmetic, no device: taps[j] = channels * fsea_fir_lowpass_taps(2 channels, 1, channels branch_taps)[j],
 *               the half-amplitude point at half a channel, scaled by M so that a row has the scale of the plan's M-point
 *               rows (a constant c gives M c in column M/2) and the dB modes' pixel mapping keeps its range.
 *   create:     channels even in [2, FSEA_PFB_MAX_CHANNELS], branch_taps in [1, FSEA_PFB_MAX_BRANCH_TAPS], oversampling q
 *               1, 2 or 4 and a divisor of channels; mode as fsea_plan_create, with its statuses (and the plan's for a size
 *               it does not serve).  A channel count that is no power of two, or below 32, runs on the plan's Bluestein
 *               path and inherits its limits: no stream capture, and the object's launches on different streams follow one
 *               another.  FSEA_EINVAL for a NULL pointer, a parameter out of range or a non-finite tap, checked before any
 *               device work; FSEA_ENODEVICE without a GPU.
 *   reset:      a zero tail and s0 = 0; synchronous.
 *   run_device: d_iq (2 n_samples bytes), d_rows (out_frames x row_bytes), d_frames (NULL, or 2 F M floats) and d_series
 *               (NULL, or 2 M F floats; FSEA_MODE_COMPLEX_F32 only), 16-byte aligned; asynchronous on `stream`.  The frames
 *               pass through the object's buffer: a call on any stream waits for the previous call of the object (an event).
 *   run_host:   the same from and to host memory through pinned staging on the object's own stream; returns when the
 *               outputs are complete.  Calls on one object from several threads are serialised.
 * Both check before any device work: FSEA_EINVAL for a NULL object or buffer (d_rows / rows only where the call yields a
 * frame), a series outside FSEA_MODE_COMPLEX_F32, a misaligned device buffer, more than 2^31 samples, F M > 2^31.
 * Destroy waits for the device. */
#define FSEA_PFB_MAX_CHANNELS 16384
#define FSEA_PFB_MAX_BRANCH_TAPS 16
int fsea_pfb_prototype(int channels, int branch_taps, double *taps);
int fsea_pfb_create(fsea_pfb **pfb, const double *taps, int channels, int branch_taps, int oversampling, int mode, int device);
int fsea_pfb_destroy(fsea_pfb *pfb);
int fsea_pfb_reset(fsea_pfb *pfb);
size_t fsea_pfb_out_frames(const fsea_pfb *pfb, size_t n_samples);
size_t fsea_pfb_row_bytes(const fsea_pfb *pfb);
int fsea_pfb_run_device(fsea_pfb *pfb, const void *d_iq, size_t n_samples, int flip, void *d_rows, void *d_frames,
                        void *d_series, void *stream);
int fsea_pfb_run_host(fsea_pfb *pfb, const uint8_t *iq, size_t n_samples, int flip, void *rows, float *frames,
                      float *series);

/* The persistence spectrum: how often was bin k at level l over all the rows offered -- what an analyser's persistence
 * display shows: the noise floor, the max-hold envelope and short bursts in one picture.  The frequency-domain twin of the
 * IQ constellation image; it consumes rows that are already resident (the FSEA_MODE_DB10_U8 / FSEA_MODE_DB5_U8_DCFIX /
 * FSEA_MODE_DB_F32 output of fsea_plan, fsea_zoom, fsea_pfb).  Integer and order-free: the counts are the same bits
 * however the rows are cut into calls.  The object owns counts[l * width + k], 256 x width uint32_t, level-major, zero after
 * create and reset; `rows`, the rows offered so far; and the f32 range (lo, hi), (-100, 0) after create, with
 * scale = (float)(256.0 / ((double)hi - (double)lo)).
 *   add:    row r starts pitch elements behind row r - 1, pitch >= width; a sub-band of wider rows is d_rows + offset with
 *           the wide pitch.  For each of the n_rows * width elements counts[level(v)][k] += 1.  U8: level = v.  F32:
 *           t = (v - lo) * scale in two rounded f32 operations (no fused multiply-add); a NaN is not counted, t < 0 gives 0,
 *           t >= 256 gives 255, otherwise (int)t.  Then rows += n_rows; a call that would take rows above 2^32 - 1 is
 *           refused, so no count can wrap.  n_rows == 0 is a successful no-op.  add_device: only the base pointer is
 *           aligned (16 bytes); asynchronous on `stream`; calls on different streams follow one another (an event).  Rows
 *           whose pitch is a multiple of 16 bytes are read 16 bytes per lane, others element by element.  add_host stages
 *           through pinned memory on the object's own stream and returns when the counts are in place.
 *           Kernels fsea_persist_u8 / fsea_persist_f32: a workgroup of 256 lanes counts a tile of 64 columns over a run of
 *           FSEA_PERSIST_RUN_ROWS rows into a 256 x 64 u32 histogram in LDS, then adds its non-zero counters to the counts.
 *   decay:  c <- floor(c * numerator / denominator) in 64-bit integers for every count, and for rows: the phosphor of a
 *           running display.  1 <= denominator, numerator <= denominator.  Asynchronous on `stream`.
 *   counts_host: the 256 * width counts, behind every add queued so far.
 *   image:  256 x width uint8_t, image[(255 - l) * width + k]: the strongest level is the top row.  full == 0 means rows; if
 *           that is 0 too the image is zero.  SATURATE: min(c, 255).  LINEAR: min(255, floor(c * 255 / full)).  LOG, integer
 *           and monotone: q(0) = 0 and for c >= 1, e = floor(log2 c), m = ((c << 8) >> e) & 255, q(c) = 256 e + m + 1; the
 *           pixel is 0 for c = 0, else min(255, 1 + floor((q(c) - 1) * 254 / max(1, q(full) - 1))): a single hit stays
 *           visible.  image_device: d_image 16-byte aligned, asynchronous on `stream`.
 *   trace:  host arithmetic on fetched counts, no device.  MAX / MIN: the highest / lowest level with a non-zero count, 0
 *           for an empty column.  QUANTILE: the smallest l whose cumulative count reaches
 *           max(1, (uint64_t)ceil(fraction * total_k)); 0.5 is the median level, the per-bin noise floor.
 * Every check runs before any device work: FSEA_EINVAL for a NULL object or buffer, a width outside
 * [1, FSEA_PERSIST_MAX_WIDTH], an unknown type, map or kind, pitch < width, n_rows > 2^31, a misaligned device pointer, a
 * range that is not finite with lo < hi (or too narrow for a finite scale), a bad decay ratio, a fraction outside [0, 1].
 * Create: FSEA_ENODEVICE without a GPU.  width and rows return 0 for NULL.  Destroy and reset wait for the device; reset
 * zeroes counts and rows and keeps the range.  Calls on one object from several threads are serialised. */
#define FSEA_PERSIST_LEVELS 256
#define FSEA_PERSIST_MAX_WIDTH 65536
#define FSEA_PERSIST_RUN_ROWS 1024   /* rows a workgroup of the add kernels counts before it adds its histogram to the counts */
enum { FSEA_PERSIST_U8 = 0, FSEA_PERSIST_F32 = 1 };                       /* element type of a row */
enum { FSEA_PERSIST_MAP_SATURATE = 0, FSEA_PERSIST_MAP_LINEAR = 1, FSEA_PERSIST_MAP_LOG = 2 };
enum { FSEA_PERSIST_TRACE_MAX = 0, FSEA_PERSIST_TRACE_MIN = 1, FSEA_PERSIST_TRACE_QUANTILE = 2 };
int fsea_persist_create(fsea_persist **persist, int width, int device);
int fsea_persist_destroy(fsea_persist *persist);
int fsea_persist_reset(fsea_persist *persist);
int fsea_persist_set_range(fsea_persist *persist, float lo, float hi);
int fsea_persist_width(const fsea_persist *persist);
uint64_t fsea_persist_rows(const fsea_persist *persist);
int fsea_persist_add_device(fsea_persist *persist, const void *d_rows, int type, size_t n_rows, size_t pitch, void *stream);
int fsea_persist_add_host(fsea_persist *persist, const void *rows, int type, size_t n_rows, size_t pitch);
int fsea_persist_decay(fsea_persist *persist, uint32_t numerator, uint32_t denominator, void *stream);
int fsea_persist_counts_host(fsea_persist *persist, uint32_t *counts);
int fsea_persist_image_device(fsea_persist *persist, int map, uint64_t full, uint8_t *d_image, void *stream);
int fsea_persist_image_host(fsea_persist *persist, int map, uint64_t full, uint8_t *image);
int fsea_persist_trace(const uint32_t *counts, int width, int kind, double fraction, uint8_t *levels);

/* The CFAR spectrum detector: which cells of a dB row hold a signal, and which bands are occupied how often -- a
 * constant-false-alarm-rate detector across frequency.  Each cell of a row is compared with the mean level of its neighbours to
 * the left and right, a few guard cells beside it left out; the per-column count of detections over many rows is the
 * occupancy (duty cycle) of the column, and runs of occupied columns are the bands.  It consumes rows that are already
 * resident (the FSEA_MODE_DB10_U8 / FSEA_MODE_DB5_U8_DCFIX / FSEA_MODE_DB_F32 output of fsea_plan, fsea_zoom, fsea_pfb, or a
 * stitched sweep image).  Integer and order-free: every result is the same bits however the rows are cut into calls.  The
 * object owns hits[k], width uint32_t, zero after create and reset; `rows`, the rows offered so far; and the settings
 * (guard G, train T, offset, method), (2, 16, 60, FSEA_CFAR_CA) after create.
 *   level:  of an element.  U8: the byte.  F32: t = v * 64 in one rounded f32 multiplication (FSEA_CFAR_F32_SCALE: 1/64 dB);
 *           a NaN gives -2^20, t <= -2^20 gives -2^20, t >= 2^20 gives 2^20, otherwise (int)rintf(t), round half to even.
 *           `offset` is in the same units: u8 levels, or 1/64 dB for f32 rows.
 *   windows: of cell k of a row of `width` cells.  Left training cells k-G-T .. k-G-1, right training cells k+G+1 .. k+G+T,
 *           each side clipped to [0, width-1], no wrap-around; nL, nR are the counts of cells and SL, SR the sums of levels.
 *   decision: for the cell's level x, all in 32-bit integers.  With ok(n, S): x*n > S + offset*n,
 *             CA (cell averaging):  nL+nR > 0 and ok(nL+nR, SL+SR)
 *             GO (greatest of):     nL+nR > 0 and every side with n > 0 satisfies ok(n, S) -- holds at the step between two
 *                                   stitched tiles
 *             SO (smallest of):     some side with n > 0 satisfies ok(n, S) -- finds the weaker of two close carriers
 *   add:    row r starts pitch elements behind row r - 1, pitch >= width; a sub-band of wider rows is d_rows + offset with the
 *           wide pitch.  d_mask (optional, NULL: not written) is tight, n_rows * width bytes, 255 for a hit and 0 otherwise.
 *           d_row_hits (optional): d_row_hits[r] is set to, not added to, the number of hits in row r of this call.
 *           hits[k] += the hits of column k; rows += n_rows; a call that would take rows above 2^32 - 1 is refused, so no
 *           count can wrap.  n_rows == 0 is a successful no-op.  The settings used are those at the time of the call.
 *           add_device: d_rows, d_mask and d_row_hits are 16-byte aligned, pitch (in elements) may be anything;
 *           asynchronous on `stream`; calls on different streams follow one another (an event).  Rows whose pitch is a
 *           multiple of 16 bytes are read 16 bytes per lane, others element by element; the mask is written 16 bytes per lane
 *           where width is a multiple of 16.  add_host stages the rows through pinned memory in chunks on the object's own
 *           stream and returns when mask, row hits and hits are in place.
 *           Kernels fsea_cfar_u8 / fsea_cfar_f32: a workgroup of 256 lanes takes a tile of FSEA_CFAR_TILE_COLUMNS columns over a
 *           run of FSEA_CFAR_RUN_ROWS rows; a row segment's prefix sums in LDS make the cost per cell independent of T.
 *   hits_host: the width hit counts, behind every add queued so far.
 *   bands:  host arithmetic on fetched hits, no device.  c_min = max(1, (uint64_t)ceil(min_fraction * rows)); column k is
 *           occupied when hits[k] >= c_min.  Going up the columns, a band runs from an occupied column through every further
 *           occupied column that has at most max_gap unoccupied columns before it; first and last are its first and last
 *           occupied columns; a band narrower than min_width columns (last - first + 1) is dropped.  peak is the lowest
 *           column of the band with the most hits, peak_hits its count, hits_sum the sum over first .. last.  rows == 0 gives
 *           no band.  At most `capacity` bands are written; *n_bands is the number found, which may exceed capacity; bands may
 *           be NULL when capacity is 0.
 * Every check runs before any device work: FSEA_EINVAL for a NULL object or input buffer, a width outside
 * [1, FSEA_CFAR_MAX_WIDTH], a guard outside [0, FSEA_CFAR_MAX_GUARD], a train outside [1, FSEA_CFAR_MAX_TRAIN], |offset| above
 * FSEA_CFAR_MAX_OFFSET, an unknown type or method, pitch < width, n_rows > 2^31, a misaligned device pointer, min_fraction
 * outside [0, 1], a negative max_gap, min_width < 1.  Create: FSEA_ENODEVICE without a GPU.  width and rows return 0 for NULL.
 * Destroy and reset wait for the device; reset zeroes hits and rows and keeps the settings.  Calls on one object from several
 * threads are serialised. */
#define FSEA_CFAR_MAX_WIDTH (1 << 20)   /* a stitched sweep image fits */
#define FSEA_CFAR_MAX_GUARD 64
#define FSEA_CFAR_MAX_TRAIN 256         /* per side */
#define FSEA_CFAR_MAX_OFFSET (1 << 20)  /* |offset| */
#define FSEA_CFAR_F32_SCALE 64          /* f32 dB rows are taken in 1/64 dB */
#define FSEA_CFAR_TILE_COLUMNS 1024     /* columns of a workgroup of the add kernels */
#define FSEA_CFAR_RUN_ROWS 64           /* rows a workgroup of the add kernels takes before it adds its column hits to hits */
enum { FSEA_CFAR_U8 = 0, FSEA_CFAR_F32 = 1 };                       /* element type of a row */
enum { FSEA_CFAR_CA = 0, FSEA_CFAR_GO = 1, FSEA_CFAR_SO = 2 };      /* method */
typedef struct {
    int32_t first, last, peak;
    uint32_t peak_hits;
    uint64_t hits_sum;
} fsea_cfar_band;
int fsea_cfar_create(fsea_cfar **cfar, int width, int device);
int fsea_cfar_destroy(fsea_cfar *cfar);
int fsea_cfar_reset(fsea_cfar *cfar);
int fsea_cfar_set(fsea_cfar *cfar, int guard, int train, int offset, int method);
int fsea_cfar_width(const fsea_cfar *cfar);
uint64_t fsea_cfar_rows(const fsea_cfar *cfar);
int fsea_cfar_add_device(fsea_cfar *cfar, const void *d_rows, int type, size_t n_rows, size_t pitch, uint8_t *d_mask,
                         uint32_t *d_row_hits, void *stream);
int fsea_cfar_add_host(fsea_cfar *cfar, const void *rows, int type, size_t n_rows, size_t pitch, uint8_t *mask,
                       uint32_t *row_hits);
int fsea_cfar_hits_host(fsea_cfar *cfar, uint32_t *hits);
int fsea_cfar_bands(const uint32_t *hits, int width, uint64_t rows, double min_fraction, int max_gap, int min_width,
                    fsea_cfar_band *bands, size_t capacity, size_t *n_bands);

/* The ordered-statistic CFAR detector: fsea_cfar's question answered against a rank of the training cells in place of their
 * mean.  A mean is pulled up by any strong neighbour, so under fsea_cfar the weaker of two close emissions gets no hit; the
 * R-th smallest level of the window is not moved by a few strong cells.  A u8 row of 128 cells at level 100 with a carrier of
 * 200 on columns 40 .. 47 and one of 130 on column 60, G = 2, T = 16, offset 20: CA hits 40 .. 47 only (column 60 sees a mean
 * of 118.75), rank 24 of 32 hits 40 .. 47 and 60.  The object is fsea_cfar's in every other respect: it owns hits[k], width
 * uint32_t, zero after create and reset; `rows`, the rows offered so far; and the settings (guard G, train T, offset, rank R),
 * (2, 16, 60, 24) after create -- three quarters of the window, Rohling's choice.  Integer and order-free.
 *   level, windows: fsea_cfar's, above: the same levels of u8 and f32 elements (FSEA_CFAR_U8 / FSEA_CFAR_F32), left training
 *           cells k-G-T .. k-G-1 and right training cells k+G+1 .. k+G+T, each side clipped to [0, width-1], no wrap-around;
 *           n = nL + nR is the number of training cells inside the row.
 *   decision: for the cell's level x, all in 32-bit integers.  r = (R*n + 2T - 1) / (2T) rounded down, that is
 *           ceil(R*n / 2T): at least 1, and R for a window that is not clipped.  z is the r-th smallest level of the n
 *           training cells, counted from 1, ties counted as often as they occur.  hit: n > 0 and x > z + offset.
 *           The counting identity: hit exactly when n > 0 and the number of training cells with level + offset < x is at
 *           least r (r such cells put the r-th smallest among them, and the r-th smallest below x - offset puts the r - 1
 *           before it there too).  This is what the kernels evaluate; nothing is sorted.
 *   set:    checks guard, train, offset, rank in this order; R is in [1, 2T].  rank returns R (0 for NULL).
 *   add, hits_host: fsea_cfar_add_* and fsea_cfar_hits_host word for word: pitch and sub-bands, the tight optional d_mask
 *           (255 / 0), the optional d_row_hits (set, not added to), hits[k] += and rows += with the 2^32 - 1 guard, the
 *           n_rows == 0 no-op, the alignment of the device form's three pointers, the order of calls on different streams, the
 *           16-byte and element-wise reads and mask writes, the staging of the host form.
 *           Kernels fsea_oscfar_u8 / fsea_oscfar_f32: a workgroup of 256 lanes takes a tile of FSEA_OSCFAR_TILE_COLUMNS columns
 *           over a run of FSEA_OSCFAR_RUN_ROWS rows; a row segment's levels in LDS are compared 2T to a cell, the cost grows
 *           with T.
 *   bands:  fsea_cfar_bands on the fetched hits.
 * Every check runs before any device work, in fsea_cfar's order with the rank behind the offset: FSEA_EINVAL for a NULL object
 * or input buffer, a width outside [1, FSEA_CFAR_MAX_WIDTH], a guard outside [0, FSEA_CFAR_MAX_GUARD], a train outside
 * [1, FSEA_CFAR_MAX_TRAIN], |offset| above FSEA_CFAR_MAX_OFFSET, a rank outside [1, 2 * train], an unknown type, pitch < width,
 * n_rows > 2^31, a misaligned device pointer.  Create: FSEA_ENODEVICE without a GPU.  width, rows and rank return 0 for NULL.
 * Destroy and reset wait for the device; reset zeroes hits and rows and keeps the settings.  Calls on one object from several
 * threads are serialised. */
#define FSEA_OSCFAR_TILE_COLUMNS 1024   /* columns of a workgroup of the add kernels */
#define FSEA_OSCFAR_RUN_ROWS 64         /* rows a workgroup of the add kernels takes before it adds its column hits to hits */
int fsea_oscfar_create(fsea_oscfar **oscfar, int width, int device);
int fsea_oscfar_destroy(fsea_oscfar *oscfar);
int fsea_oscfar_reset(fsea_oscfar *oscfar);
int fsea_oscfar_set(fsea_oscfar *oscfar, int guard, int train, int offset, int rank);
int fsea_oscfar_width(const fsea_oscfar *oscfar);
uint64_t fsea_oscfar_rows(const fsea_oscfar *oscfar);
int fsea_oscfar_rank(const fsea_oscfar *oscfar);
int fsea_oscfar_add_device(fsea_oscfar *oscfar, const void *d_rows, int type, size_t n_rows, size_t pitch, uint8_t *d_mask,
                           uint32_t *d_row_hits, void *stream);
int fsea_oscfar_add_host(fsea_oscfar *oscfar, const void *rows, int type, size_t n_rows, size_t pitch, uint8_t *mask,
                         uint32_t *row_hits);
int fsea_oscfar_hits_host(fsea_oscfar *oscfar, uint32_t *hits);

/* The time-axis CFAR detector: fsea_cfar's question put down each column.  fsea_cfar and fsea_oscfar compare a cell with its
 * neighbours in the same row, so a cell inside a flat-topped emission wider than the window sees only the emission and gets no
 * hit: 64 u8 rows of 256 cells at level 100, a burst of 160 on rows 30 .. 35 and columns 40 .. 199, a carrier of 200 on column
 * 220, G = 2, T = 16, offset 20, CA: fsea_cfar hits the burst's two edges (columns 40 .. 47 and 192 .. 199) and the carrier in
 * all 64 rows; fsea_tcfar hits all 960 cells of the burst and no cell of the carrier.  Here a cell is compared with the cells
 * of the same column in the rows before and after it.  The object is fsea_cfar's in every other respect: it owns hits[k],
 * width uint32_t, zero after create and reset; `rows`, the rows decided so far; and the settings (guard G, train T, offset,
 * method, mask operation), (2, 16, 60, FSEA_CFAR_CA, FSEA_TCFAR_MASK_SET) after create.  Integer and order-free.  It carries no
 * state from call to call other than hits and rows.
 *   level:  of an element: fsea_cfar's, above (FSEA_CFAR_U8 and FSEA_CFAR_F32).
 *   rows:   of a call.  A call decides n_rows rows; d_rows points at the first decided row.  rows_before further rows lie in
 *           memory in front of it, at the same pitch, and rows_after rows behind the last decided row: the context.  The rows
 *           of the call are numbered -rows_before .. n_rows + rows_after - 1.
 *   windows: of cell (r, k).  Earlier training cells: rows r-G-T .. r-G-1 of column k; later training cells: rows r+G+1 ..
 *           r+G+T; each side clipped to the rows of the call, no wrap-around; nL, nR are the counts of cells and SL, SR the
 *           sums of levels.  G and T are counted in rows.  Context beyond G + T rows on a side is never read.
 *   decision: fsea_cfar's ok(n, S) and its three methods with nL, SL, nR, SR as above, in 32-bit integers (|S| <= 256 * 2^20).
 *           In time, GO holds at a level step (a retune); SO finds the onset and the end of a long emission.
 *           In one sentence: the mask of a call is fsea_cfar's mask of the transposed block of rows_before + n_rows +
 *           rows_after rows, transposed back, rows 0 .. n_rows - 1 kept.
 *   cuts:   a recording decided in any number of calls gives the same bits as one call over all of it when every call gets
 *           min(G + T, the rows that exist) rows of context on each side.
 *   mask operation: FSEA_TCFAR_MASK_SET: the mask byte becomes 255 for a hit and 0 otherwise.  FSEA_TCFAR_MASK_OR and
 *           FSEA_TCFAR_MASK_AND combine the decision with what d_mask already holds, any non-zero byte counting as set; the
 *           result is written as 255 or 0.  hits, d_row_hits and the mask all describe the written value.  fsea_cfar or
 *           fsea_oscfar writes a mask, then fsea_tcfar with OR gives "either axis" and with AND "stands out on both".
 *   set:    checks guard, train, offset (fsea_cfar's ranges), method, mask operation in this order.
 *   run_rows: the rows a workgroup of the add kernels decides under the current settings, FSEA_TCFAR_RUN_ROWS whatever they
 *           are (0 for NULL): where the seams of a call lie.
 *   add, hits_host: fsea_cfar_add_* and fsea_cfar_hits_host with the context rows: pitch and sub-bands, the tight d_mask of
 *           n_rows * width bytes (optional under SET, read and written under OR and AND), the optional d_row_hits (set, not
 *           added to), hits[k] += and rows += n_rows with the 2^32 - 1 guard, the n_rows == 0 no-op, the alignment of the
 *           device form's three pointers, the order of calls on different streams, the 16-byte and element-wise reads and
 *           mask accesses.  add_host: `rows` points at the first decided row of the caller's array, the context rows around
 *           it; the rows go up in chunks, each with its context rows and, where the operation reads it, its mask, so the
 *           host form equals the device form bit for bit.  A row so long that 2 (G + T) + 1 packed rows do not fit the
 *           staging of 64 MiB is refused: use add_device.
 *           Kernels fsea_tcfar_u8 / fsea_tcfar_f32: a workgroup of one wave takes a tile of FSEA_TCFAR_TILE_COLUMNS columns
 *           over a run of FSEA_TCFAR_RUN_ROWS rows; a lane keeps the window sums of its 16 columns in registers and moves
 *           them on with five row reads per row, the cost per cell independent of T.
 *   bands:  fsea_cfar_bands on the fetched hits.
 * Every check runs before any device work, in this order: FSEA_EINVAL for a NULL object, an unknown type, n_rows > 2^31, a
 * NULL input buffer, pitch < width, (rows_before + n_rows + rows_after) x pitch above 2^40, a misaligned device pointer, OR or
 * AND without a mask, rows past 2^32 - 1.  Create: FSEA_ENODEVICE without a GPU.  width, rows and run_rows return 0 for NULL.
 * Destroy and reset wait for the device; reset zeroes hits and rows and keeps the settings.  Calls on one object from several
 * threads are serialised. */
#define FSEA_TCFAR_TILE_COLUMNS 1024    /* columns of a workgroup of the add kernels */
#define FSEA_TCFAR_RUN_ROWS 32          /* rows a workgroup of the add kernels decides before it adds its column hits to hits */
enum { FSEA_TCFAR_MASK_SET = 0, FSEA_TCFAR_MASK_OR = 1, FSEA_TCFAR_MASK_AND = 2 };   /* mask operation */
int fsea_tcfar_create(fsea_tcfar **tcfar, int width, int device);
int fsea_tcfar_destroy(fsea_tcfar *tcfar);
int fsea_tcfar_reset(fsea_tcfar *tcfar);
int fsea_tcfar_set(fsea_tcfar *tcfar, int guard, int train, int offset, int method, int mask_op);
int fsea_tcfar_width(const fsea_tcfar *tcfar);
uint64_t fsea_tcfar_rows(const fsea_tcfar *tcfar);
int fsea_tcfar_run_rows(const fsea_tcfar *tcfar);
int fsea_tcfar_add_device(fsea_tcfar *tcfar, const void *d_rows, int type, size_t n_rows, size_t pitch, size_t rows_before,
                          size_t rows_after, uint8_t *d_mask, uint32_t *d_row_hits, void *stream);
int fsea_tcfar_add_host(fsea_tcfar *tcfar, const void *rows, int type, size_t n_rows, size_t pitch, size_t rows_before,
                        size_t rows_after, uint8_t *mask, uint32_t *row_hits);
int fsea_tcfar_hits_host(fsea_tcfar *tcfar, uint32_t *hits);

/* Spectrum events: which emissions a detection mask holds -- this burst, from row 812 to row 860, columns 3011 .. 3042, peak
 * 171 at (830, 3027).  A device pass reduces a resident mask (fsea_cfar's, n_rows x width bytes) and optionally the level rows
 * under it to a sorted list of runs, a few records per row; fsea_events_link joins the runs into events on the host; a device
 * pass paints runs back as a cleaned mask or a label image.  Integer and bit for bit: every record is the same whatever the
 * launch geometry or the cut of the rows into calls.  The object owns `rows`, the rows offered since create or reset, and the
 * column gap G, 0 after create.
 *   hit:    a mask byte that is not 0 (fsea_cfar writes 255).
 *   level:  of a cell: fsea_cfar's, above.  FSEA_CFAR_U8: the byte.  FSEA_CFAR_F32: rint(v * 64) in one rounded f32
 *           multiplication, clamped to +-2^20, -2^20 for a NaN.
 *   runs:   of a row.  Going up the columns, a run starts at a hit and continues through every further hit that has at most G
 *           non-hit columns before it (fsea_cfar_bands' wording).  One record per run: row = rows at the call + the row within
 *           the call; first and last, its first and last hit column; hits, the hit cells in first .. last (last - first + 1
 *           when G is 0); peak, the largest level over the hit cells, and peak_col, the lowest hit column that holds it;
 *           level_sum, the sum of the levels over the hit cells.  Without level rows (d_levels NULL; `type` is still checked)
 *           peak = 0, peak_col = first, level_sum = 0.  The records come out sorted by (row, first).  At most `capacity` are
 *           written, the first ones in order; *n_runs is the number found, which may exceed capacity; capacity 0 with a NULL
 *           buffer just counts.  Then rows += n_rows; a call that would take rows past 2^32 - 1 is refused.  n_rows == 0 is
 *           a successful no-op with *n_runs = 0.  Row r of the mask starts mask_pitch bytes behind row r - 1, of the levels
 *           level_pitch elements; both pitches >= width.  runs_device: d_mask, d_levels and d_runs are 16-byte aligned;
 *           queued on `stream`, and the call waits for its own count before it returns: the records are then in place.
 *           Rows whose pitches are multiples of 16 bytes are read 16 bytes per lane, others element by element; no load
 *           passes the width of a row, no store the capacity.  runs_host stages mask and levels through pinned memory in
 *           chunks of rows on the object's own stream.
 *           Kernels fsea_events_count and fsea_events_runs / _u8 / _f32 (and their _narrow forms): one wave per row walks
 *           it in chunks of 64 lanes x 16 cells with a carry; the first pass counts the runs of every row, a scan over the
 *           rows gives each row's first index and the total, the second pass stores the records: sorted without a sort.
 *   touch:  run a in row ra and run b in row rb > ra touch when rb - ra <= gap_rows + 1, first_a <= last_b + gap_cols and
 *           first_b <= last_a + gap_cols.  With both gaps 0 this is 4-connectivity on the mask.
 *   link:   host arithmetic, no device.  The events are the connected components of the touch relation.  An event's record:
 *           the box row_first .. row_last, col_first .. col_last; runs; hits; peak with peak_row and peak_col, ties to the
 *           lowest row, then the lowest column; level_sum, wrapping modulo 2^64.  The events are ordered by the position of
 *           their first run in the list.  An event whose box is lower than min_rows or narrower than min_cols, or whose hits
 *           are below min_hits, is dropped; the survivors are numbered 0, 1, ... in order.  event_of_run[i] (optional) is the
 *           number of run i's event, FSEA_EVENTS_NO_EVENT for a run of a dropped one.  At most `capacity` events are written;
 *           *n_events is the number that survive; events may be NULL when capacity is 0.  The runs must be sorted by
 *           (row, first), disjoint within a row, first <= last.  The cost is linear in the runs and the pairs that touch.
 *   paint:  every byte of the n_rows x width image (row r starts pitch bytes behind row r - 1, pitch >= width; the bytes
 *           between width and pitch are left alone) is written: columns first .. last of a run with values[i] != 0 hold
 *           values[i], closed gaps included, everything else 0.  Image row 0 is row `row0`; runs whose row lies outside
 *           [row0, row0 + n_rows), and runs that do not lie inside the width, are ignored.  Runs that overlap are the
 *           caller's error.  paint_device: d_runs and d_image 16-byte aligned, asynchronous on `stream`.
 *           Kernel fsea_events_paint: a zero fill, then one wave per run, 16-byte stores in the aligned middle.
 * Every check runs before any device work: FSEA_EINVAL for a NULL object, buffer or count, a width outside
 * [1, FSEA_EVENTS_MAX_WIDTH], a gap_cols outside [0, FSEA_EVENTS_MAX_GAP_COLS], a gap_rows outside
 * [0, FSEA_EVENTS_MAX_GAP_ROWS], an unknown type, a pitch < width, n_rows > 2^31, a misaligned device pointer, a filter
 * below 1, runs that are not sorted.  Create: FSEA_ENODEVICE without a GPU.  width and rows return 0 for NULL.  Destroy and
 * reset wait for the device; reset puts rows back to 0 and keeps the gap.  Calls on one object from several threads are
 * serialised. */
#define FSEA_EVENTS_MAX_WIDTH (1 << 20)
#define FSEA_EVENTS_MAX_GAP_COLS 64
#define FSEA_EVENTS_MAX_GAP_ROWS (1 << 16)
#define FSEA_EVENTS_NO_EVENT 0xFFFFFFFFu
typedef struct {            /* 32 bytes */
    uint32_t row;
    uint32_t first, last;
    uint32_t hits;
    int32_t peak;
    uint32_t peak_col;
    int64_t level_sum;
} fsea_events_run;
typedef struct {            /* 48 bytes */
    uint32_t row_first, row_last, col_first, col_last;
    uint32_t runs;
    int32_t peak;
    uint32_t peak_row, peak_col;
    uint64_t hits;
    int64_t level_sum;
} fsea_events_event;
int fsea_events_create(fsea_events **events, int width, int device);
int fsea_events_destroy(fsea_events *events);
int fsea_events_reset(fsea_events *events);
int fsea_events_set_gap(fsea_events *events, int gap_cols);
int fsea_events_width(const fsea_events *events);
uint64_t fsea_events_rows(const fsea_events *events);
int fsea_events_runs_device(fsea_events *events, const uint8_t *d_mask, size_t mask_pitch, const void *d_levels, int type,
                            size_t level_pitch, size_t n_rows, fsea_events_run *d_runs, size_t capacity, size_t *n_runs,
                            void *stream);
int fsea_events_runs_host(fsea_events *events, const uint8_t *mask, size_t mask_pitch, const void *levels, int type,
                          size_t level_pitch, size_t n_rows, fsea_events_run *runs, size_t capacity, size_t *n_runs);
int fsea_events_link(const fsea_events_run *runs, size_t n_runs, int gap_cols, int gap_rows, uint32_t min_rows,
                     uint32_t min_cols, uint64_t min_hits, uint32_t *event_of_run, fsea_events_event *events, size_t capacity,
                     size_t *n_events);
int fsea_events_paint_device(fsea_events *events, const fsea_events_run *d_runs, const uint8_t *d_values, size_t n_runs,
                             uint64_t row0, size_t n_rows, uint8_t *d_image, size_t pitch, void *stream);
int fsea_events_paint_host(fsea_events *events, const fsea_events_run *runs, const uint8_t *values, size_t n_runs, uint64_t row0,
                           size_t n_rows, uint8_t *image, size_t pitch);

/* Event cut-outs: the signal behind each box of fsea_events_link -- the emission's IQ mixed to the centre, low-passed to its
 * own bandwidth and decimated.  fsea_zoom does this arithmetic for one centre frequency and one contiguous stream per call;
 * an event list is hundreds of short spans, each with its own centre and start, scattered over one resident recording.  An
 * fsea_extract holds the taps c (L of them) and the decimation D and takes a table of jobs over one resident buffer of 8-bit
 * IQ: every job's decimated pairs in one launch.  There is no state between calls and no reset.
 *   job:        with x the rotated samples of fsea_fir_u8_shifted_* for the n_samples samples at d_iq + 2 first (same flip; the
 *               stream position of sample m is sample_offset + m; cycles_per_sample and phase0_cycles the job's own) and
 *               x_ext = (L - 1 zeros) ++ x,
 *                 pairs[out_first + i] = sum_{k < L} c[k] x_ext[i D + k],   i < n_samples / D (rounded down):
 *               the pairs fsea_zoom_run_device writes right after fsea_zoom_reset with the same taps, D, flip and arguments
 *               on those samples, bit for bit, whatever other jobs share the call, whatever their order and whatever first
 *               mod 8 is.  Jobs may overlap in the input; their output ranges must not overlap and lie inside
 *               pairs_capacity.  A job with n_samples < D has no output and is legal.  Nothing outside the jobs' output
 *               ranges is written, nothing outside the n_iq_samples samples is read.  `jobs` is host memory, read before
 *               the call returns.  first and sample_offset are two fields because a caller that uploads only a window of a
 *               recording rebases first and leaves the stream position alone.
 *   create:     taps and decimation as fsea_zoom_create, with its limits (FSEA_FIR_MAX_TAPS, FSEA_ZOOM_MAX_DECIMATION) and
 *               checks; FSEA_ENODEVICE without a GPU.  decimation and n_taps return 0 for NULL, out_pairs (n_samples / D) too.
 *   lead:       ceil((L - 1) / D) D, the samples in front of an event a job starts early so that output lead / D is the first
 *               whose taps all lie on samples; 0 for an n_taps or decimation below 1.  No object needed.
 *   layout:     fills out_first in job order, each job at the next even pair index (a 16-byte boundary), and gives the
 *               capacity needed in *total_pairs.  FSEA_EINVAL for a NULL object or total_pairs, n_jobs above
 *               FSEA_EXTRACT_MAX_JOBS, a NULL table with n_jobs > 0.
 *   run_device: d_iq (2 n_iq_samples bytes) and d_pairs (2 pairs_capacity floats) 16-byte aligned; asynchronous on `stream`.
 *               The object owns the device table of the jobs, so calls on several streams follow one another (an event).
 *               Kernel fsea_extract_u8 (and _s, _m: the zoom's three LDS sizes): one workgroup per tile of
 *               FSEA_ZOOM_TILE_OUTPUTS outputs of one job, which it finds by a bisection over the jobs' first tiles.
 *   run_host:   the same from and to host memory through pinned staging on the object's own stream; returns when `pairs` is
 *               complete; of `pairs` only the jobs' output ranges are written.
 * Both check, before any device work and reading nothing of the object but its decimation, in this order: a NULL object;
 * n_jobs above FSEA_EXTRACT_MAX_JOBS; n_jobs == 0 is then a successful no-op; a NULL job table; a NULL buffer; per job in
 * table order: first + n_samples past n_iq_samples, n_samples above 2^31, the cycles_per_sample, phase0_cycles and
 * sample_offset + n_samples limits of fsea_fir_u8_shifted_* (each text names the job); more than 2^31 outputs in the call;
 * per job with output in table order: an output range past pairs_capacity; two output ranges that overlap (the text names
 * both jobs); for run_device a misaligned d_iq or d_pairs.  All FSEA_EINVAL; a refused call writes nothing.  Destroy waits
 * for the device.  Calls on one object from several threads are serialised.
 *   jobs:       fsea_extract_jobs, host arithmetic, no device: one job per event, in order.  With N = width, H = hop, row r of
 *               the events beginning at sample r H of a recording of n_samples samples, and lead as above: begin =
 *               row_first H; first = sample_offset = begin - min(begin, lead); end = min(n_samples, row_last H + N); the
 *               job's n_samples = end - first, 0 if end <= first; cycles_per_sample = -(col_first + col_last - 2 (N / 2)) /
 *               (2 N): the negated integer over the integer 2 N in one double division (column N / 2 is the centre; an
 *               event centred there gets +0.0); phase0_cycles = 0; out_first = 0, the caller lays the jobs out.  fits[i] =
 *               1 when (col_last - col_first + 1) D <= max_fill N (the product max_fill N rounded once), else 0 and the
 *               job's n_samples 0.  FSEA_EINVAL for NULL pointers (with n_events > 0), width or hop < 1, n_taps or
 *               decimation out of create's range, max_fill outside (0, 1]. */
#define FSEA_EXTRACT_MAX_JOBS 65536
typedef struct {              /* 48 bytes */
    uint64_t first;           /* index in d_iq / iq of the job's sample 0 */
    uint64_t n_samples;       /* samples of the job, <= 2^31; first + n_samples <= n_iq_samples */
    uint64_t sample_offset;   /* stream position of the job's sample 0 (the phase; as fsea_fir_u8_shifted_*) */
    double cycles_per_sample;
    double phase0_cycles;
    uint64_t out_first;       /* index in d_pairs / pairs of the job's output 0; it has n_samples / D outputs */
} fsea_extract_job;
int fsea_extract_create(fsea_extract **extract, const double *taps, int n_taps, int decimation, int device);
int fsea_extract_destroy(fsea_extract *extract);
int fsea_extract_decimation(const fsea_extract *extract);
int fsea_extract_n_taps(const fsea_extract *extract);
size_t fsea_extract_out_pairs(const fsea_extract *extract, size_t n_samples);
size_t fsea_extract_lead(int n_taps, int decimation);
int fsea_extract_layout(const fsea_extract *extract, fsea_extract_job *jobs, size_t n_jobs, size_t *total_pairs);
int fsea_extract_run_device(fsea_extract *extract, const void *d_iq, size_t n_iq_samples, int flip, const fsea_extract_job *jobs,
                            size_t n_jobs, void *d_pairs, size_t pairs_capacity, void *stream);
int fsea_extract_run_host(fsea_extract *extract, const uint8_t *iq, size_t n_iq_samples, int flip, const fsea_extract_job *jobs,
                          size_t n_jobs, float *pairs, size_t pairs_capacity);
int fsea_extract_jobs(const fsea_events_event *events, size_t n_events, int width, int hop, uint64_t n_samples, int n_taps,
                      int decimation, double max_fill, fsea_extract_job *jobs, uint8_t *fits);

/* Signal measures: what is inside each cut-out -- how strong it is, how far it sits from the centre its box gave it, how wide
 * it is, whether its envelope is constant (FM, FSK, a carrier) or noise-like (OFDM, DVB-T).  All of it follows from a few
 * sums per cut-out, the pulse-pair moments of radar plus the envelope's second and fourth moments.  An fsea_measure takes a
 * table of jobs over one resident buffer of f32 pairs (what fsea_extract_run_device left) and gives one record of sums per
 * job, in one launch for the tiles and one for the fold.  There is no state between calls and no reset.
 *   terms:      for pair i of a job, z_i = pairs[first_pair + i], in f64 with exactly the roundings written here (rn = one
 *               IEEE rounding; nothing is contracted into an FMA):
 *                 a_i = rn((double)re_i - offset_re),   b_i = rn((double)im_i - offset_im),
 *                 P_i = rn(rn(a_i a_i) + rn(b_i b_i)),  Q_i = rn(P_i P_i),   and with j = i - lag, for i >= lag,
 *                 Rre_i = rn(rn(a_i a_j) + rn(b_i b_j)),  Rim_i = rn(rn(b_i a_j) - rn(a_i b_j));
 *               for i < lag both R terms are +0.0 and keep their place in the order.  offset is the pedestal the caller
 *               knows: a cut-out rests on (0.5 + 0.5j) sum(c), and what is left of it shows in s_re, s_im.
 *   order:      fold_W(x[0 .. m)): W accumulators start at +0.0; accumulator l adds x[l], x[l + W], x[l + 2 W], ... in that
 *               order; then for k = 1, 2, 4, ..., W / 2: acc[l] = acc[l] + acc[l ^ k] for every l; the value is acc[0]; an
 *               absent x counts as +0.0.  A job's pairs are cut into tiles of FSEA_MEASURE_TILE_PAIRS counted from the job's
 *               own pair 0.  A tile's partial of each of the six sums (a_i, b_i, P_i, Q_i, Rre_i, Rim_i) is fold_256 over the
 *               tile's terms; a job's sum is fold_64 over its tiles' partials in tile order.  peak is the largest P_i
 *               (comparisons: a NaN term is never the peak), peak_index the least i that has it.  Nothing in this depends on
 *               first_pair (at any parity), on the other jobs, on their order or on the launch geometry: a job's record is
 *               the same bits alone or in a table of FSEA_MEASURE_MAX_JOBS.
 *   table:      jobs may overlap and may repeat; sums[k] belongs to jobs[k]; an empty job gets zeros, peak +0.0 and
 *               peak_index 0.  `jobs` is host memory, read before the call returns.  Only the jobs' pairs are read, only the
 *               n_jobs records are written.
 *   create:     FSEA_ENODEVICE without a GPU.  Destroy waits for the device.
 *   run_device: d_pairs (n_buffer_pairs pairs of floats) 8-byte aligned, d_sums (n_jobs records) 16-byte aligned;
 *               asynchronous on `stream`.  The object owns the device copy of the table and the tile partials and grows them
 *               as needed, so calls on several streams follow one another (an event).  Kernel fsea_measure_tiles: one
 *               workgroup per tile of one job, which it finds by a bisection over the jobs' first tiles; kernel
 *               fsea_measure_fold: one wave per job.
 *   run_host:   the same from and to host memory through pinned staging on the object's own stream; returns when `sums` is
 *               complete.
 * Both check, before any device work and reading nothing of the object, in this order: a NULL object; n_jobs above
 * FSEA_MEASURE_MAX_JOBS; n_jobs == 0 is then a successful no-op; a NULL job table; a NULL buffer (pairs or sums); lag outside
 * [1, FSEA_MEASURE_MAX_LAG]; an offset that is not finite; per job in table order: first_pair + n_pairs past n_buffer_pairs,
 * n_pairs above FSEA_MEASURE_MAX_PAIRS (each text names the job); more than 2^31 pairs in the call; for run_device a d_pairs
 * that is not 8-byte or a d_sums that is not 16-byte aligned.  All FSEA_EINVAL; a refused call writes nothing.  Calls on one
 * object from several threads are serialised.
 *   jobs:       fsea_measure_jobs, host arithmetic, no device: the spans of the outputs of extract jobs that were laid out
 *               (fsea_extract_layout), without the first skip_pairs of each (the filter's run-in, fsea_extract_lead /
 *               decimation).  With outs = n_samples / decimation (rounded down) and skip = min(skip_pairs, outs): job k
 *               gets first_pair = out_first + skip, n_pairs = outs - skip.  FSEA_EINVAL for NULL tables with n_jobs > 0,
 *               n_jobs above FSEA_MEASURE_MAX_JOBS, decimation < 1, a span longer than FSEA_MEASURE_MAX_PAIRS (the text
 *               names the job).
 *   finish:     fsea_measure_finish, host arithmetic, callable in a process without a GPU: one record of sums and the lag
 *               it was made with to the measures, with n = n_pairs, m = n_lagged and |r| = hypot(r_re, r_im):
 *                 mean_power   = p / n                       power_db = 10 log10(mean_power)
 *                 dc_re, dc_im = s_re / n, s_im / n
 *                 freq_cycles  = atan2(r_im, r_re) / (2 pi lag)      cycles per pair, unambiguous within +-1 / (2 lag)
 *                 coherence    = rho = min(1, |r| n / (p m))
 *                 width_cycles = sqrt(-2 ln rho) / (2 pi lag)        the pulse-pair width of a Gaussian spectrum
 *                 kurtosis     = n q / p^2                   1 for a constant envelope, 2 for complex Gaussian noise
 *                 crest        = peak n / p
 *                 peak_index   = the sums' own
 *               With n == 0 or p == 0 the ratios are NaN (power_db of a zero mean power is -inf) and the call still returns
 *               FSEA_OK; freq_cycles, coherence and width_cycles are NaN when m == 0.  FSEA_EINVAL for a NULL pointer or a
 *               lag outside [1, FSEA_MEASURE_MAX_LAG]. */
#define FSEA_MEASURE_TILE_PAIRS 4096
#define FSEA_MEASURE_MAX_JOBS   65536          /* = FSEA_EXTRACT_MAX_JOBS */
#define FSEA_MEASURE_MAX_PAIRS  (1u << 24)     /* per job */
#define FSEA_MEASURE_MAX_LAG    65536
typedef struct { uint64_t first_pair, n_pairs; } fsea_measure_job;       /* 16 bytes */
typedef struct {                                                        /* 80 bytes */
    double s_re, s_im;      /* sum z                          */
    double p;               /* sum |z|^2                      */
    double q;               /* sum |z|^4                      */
    double r_re, r_im;      /* sum z[i] conj(z[i - lag]), i >= lag */
    double peak;            /* max |z|^2                      */
    uint64_t peak_index;    /* first i that has it (0 for an empty job) */
    uint64_t n_pairs, n_lagged;   /* n, max(n - lag, 0)       */
} fsea_measure_sums;
typedef struct {                                                        /* 88 bytes */
    double mean_power, power_db;
    double dc_re, dc_im;
    double freq_cycles;
    double coherence, width_cycles;
    double kurtosis, crest;
    uint64_t peak_index;
    uint64_t n_pairs;
} fsea_measure_result;
typedef struct fsea_measure fsea_measure;
int fsea_measure_create(fsea_measure **m, int device);
int fsea_measure_destroy(fsea_measure *m);
int fsea_measure_run_device(fsea_measure *m, const void *d_pairs, size_t n_buffer_pairs, const fsea_measure_job *jobs,
                            size_t n_jobs, double offset_re, double offset_im, int lag, fsea_measure_sums *d_sums, void *stream);
int fsea_measure_run_host(fsea_measure *m, const float *pairs, size_t n_buffer_pairs, const fsea_measure_job *jobs,
                          size_t n_jobs, double offset_re, double offset_im, int lag, fsea_measure_sums *sums);
int fsea_measure_jobs(const fsea_extract_job *ejobs, size_t n_jobs, int decimation, size_t skip_pairs, fsea_measure_job *jobs);
int fsea_measure_finish(const fsea_measure_sums *sums, int lag, fsea_measure_result *result);

/* Cut-out audio: what each cut-out carries -- the FM discriminator of the reference's WBFM chain or the AM envelope, then a
 * real low-pass that keeps every D-th value.  fsea_demod does this for one continuous 8-bit stream at the reference's fixed
 * rates, with state from call to call; an event list is hundreds of short cut-outs that already lie resident as centred,
 * band-limited f32 pairs (what fsea_extract_run_device left).  An fsea_audio holds the kind, L real f64 taps c and the
 * decimation D, takes a table of jobs over that buffer and gives every job's audio in one launch.  There is no state between
 * calls and no reset.
 *   terms:      for pair i of a job, z_i = pairs[first_pair + i], in f64 with exactly the roundings written here (rn = one
 *               IEEE rounding, round to nearest even; nothing is contracted into an FMA; / and sqrt are correctly rounded):
 *                 a_i = rn((double)re_i - offset_re),   b_i = rn((double)im_i - offset_im);
 *               offset is the pedestal the caller knows, (0.5 + 0.5j) sum(c) of the extract's taps, as for the measures.
 *   FM:         d_0 = +0.0: the first pair has none before it.  For i >= 1, with (a', b') = (a_(i-1), b_(i-1)):
 *                 real = rn(rn(a' a) + rn(b' b)),   imag = rn(rn(a' b) - rn(a b')),
 *               then the reference's arctangent (src/nrf.c:971-991) without its ampl_conv factor: sgn = +1; if imag < 0:
 *               sgn = -1, imag = -imag.  If real == imag: ang = 0, div = 1; else if real > imag: ang = 0, div = rn(imag /
 *               real); else: ang = -pi / 2 (the double nearest to it), div = rn(real / imag), sgn = -sgn.
 *                 d_i = sgn rn(ang + rn(div / rn(0.98419158358617365 + rn(div rn(0.093485702629671305 +
 *                                                                              rn(div 0.19556307900617517))))))
 *               One deviation from the reference: where real and imag are both zero (either sign) d_i = +0.0; the reference's
 *               real == imag branch gives 0.785 for a silent pair.  A NaN or an infinity in a pair gives what these
 *               expressions and comparisons give: with a NaN no comparison holds, the third branch divides and d_i is NaN.
 *               d is in radians per pair.  The expression is the reference's and so is its error: within 9.4e-4 of
 *               atan2(imag, real) for a phase step of at most a quarter turn (real >= 0); behind that it falls away from
 *               the angle, 0.14 off at three eighths of a turn and pi / 2 off at half a turn.  An emission belongs in the
 *               inner half of the cut-out's band: offset plus deviation below a quarter of the pair rate.
 *   AM:         d_i = sqrt(rn(rn(a_i a_i) + rn(b_i b_i))) for every i.
 *   filter:     with d_ext = (L - 1 values of +0.0) ++ d, output j of a job of n pairs, j < n / D (rounded down):
 *                 acc = +0.0;  for k = 0 .. L - 1 ascending: acc = rn(acc + rn(c[k] d_ext[j D + k]));
 *                 audio[out_first + j] = (float) rn(gain acc)      (the conversion rounds to nearest even).
 *               An accumulator is never -0.0: it starts at +0.0, and a sum in round-to-nearest is -0.0 only when both of its
 *               operands are -0.0.  So a term rn(c[k] (+0.0)) = +-0.0 of the zero prefix leaves it as it is and may be added
 *               or left out: the same bits.
 *               An output depends on the job's pairs alone: not on first_pair (at any parity), on the other jobs, on their
 *               order, on the tile size or on the launch geometry.
 *   table:      jobs may overlap and may repeat in the input; their output ranges must not overlap and lie inside n_audio.
 *               A job with n_pairs < D (an empty one too) has no output, writes nothing and is legal.  Only the jobs' pairs
 *               are read, only the jobs' outputs are written.  `jobs` is host memory, read before the call returns.
 *   create:     kind FSEA_AUDIO_FM or FSEA_AUDIO_AM; 1 .. FSEA_FIR_MAX_TAPS finite taps, kept as f64 on the device;
 *               decimation in [1, FSEA_AUDIO_MAX_DECIMATION].  FSEA_EINVAL, in this order, for a NULL out-pointer, another
 *               kind, NULL taps, n_taps out of range, a tap that is not finite, decimation out of range; only then
 *               FSEA_ENODEVICE without a GPU.  kind returns -1 for NULL, decimation and n_taps 0.  Destroy waits for the device.
 *   layout:     fills out_first back to back in table order (job k's n_pairs / D outputs behind job k - 1's) and gives the
 *               floats needed in *total_outputs.  FSEA_EINVAL for a NULL object or total_outputs, n_jobs above
 *               FSEA_AUDIO_MAX_JOBS, a NULL table with n_jobs > 0.
 *   run_device: d_pairs (n_buffer_pairs pairs of floats) 8-byte aligned, d_audio (n_audio floats) 4-byte aligned;
 *               asynchronous on `stream`.  The object owns the device copy of the table, so calls on several streams follow
 *               one another (an event).  A call is one upload of the table and one launch of fsea_audio_tiles: one workgroup
 *               per tile of T outputs of one job, which it finds by a bisection over the jobs' first tiles; T is the largest
 *               count up to 256 for which T D + L - 1 <= 4096, a constant of the object that no output depends on.
 *   run_host:   the same from and to host memory through pinned staging on the object's own stream; returns when `audio` is
 *               complete; of `audio` only the jobs' output ranges are written.
 * Both check, before any device work and reading nothing of the object but its decimation, in this order: a NULL object;
 * n_jobs above FSEA_AUDIO_MAX_JOBS; n_jobs == 0 is then a successful no-op; a NULL job table; a NULL buffer (pairs or audio);
 * an offset that is not finite; a gain that is not finite; per job in table order: first_pair + n_pairs past n_buffer_pairs,
 * n_pairs above FSEA_AUDIO_MAX_PAIRS, for a job with output out_first + n_pairs / D past n_audio (each text names the job);
 * two output ranges that overlap (the text names both jobs); more than 2^31 outputs in the call; for run_device a d_pairs
 * that is not 8-byte or a d_audio that is not 4-byte aligned.  All FSEA_EINVAL; a refused call writes nothing.  Calls on one
 * object from several threads are serialised. */
#define FSEA_AUDIO_FM 0
#define FSEA_AUDIO_AM 1
#define FSEA_AUDIO_MAX_DECIMATION 64
#define FSEA_AUDIO_MAX_JOBS  65536        /* = FSEA_EXTRACT_MAX_JOBS */
#define FSEA_AUDIO_MAX_PAIRS (1u << 24)   /* per job */
typedef struct { uint64_t first_pair, n_pairs, out_first; } fsea_audio_job;   /* 24 bytes */
typedef struct fsea_audio fsea_audio;
int fsea_audio_create(fsea_audio **audio, int kind, const double *taps, int n_taps, int decimation, int device);
int fsea_audio_destroy(fsea_audio *audio);
int fsea_audio_kind(const fsea_audio *audio);
int fsea_audio_decimation(const fsea_audio *audio);
int fsea_audio_n_taps(const fsea_audio *audio);
int fsea_audio_layout(const fsea_audio *audio, fsea_audio_job *jobs, size_t n_jobs, size_t *total_outputs);
int fsea_audio_run_device(fsea_audio *audio, const void *d_pairs, size_t n_buffer_pairs, const fsea_audio_job *jobs, size_t n_jobs,
                          double offset_re, double offset_im, double gain, float *d_audio, size_t n_audio, void *stream);
int fsea_audio_run_host(fsea_audio *audio, const float *pairs, size_t n_buffer_pairs, const fsea_audio_job *jobs, size_t n_jobs,
                        double offset_re, double offset_im, double gain, float *audio_out, size_t n_audio);

/* Cut-out spectra: what each cut-out looks like in frequency -- the averaged periodogram of the cut-out itself, or of one of
 * the three nonlinear forms that tell emissions apart: |z|^2, whose line sits at the symbol rate; z^2, whose line sits at
 * twice the carrier offset for BPSK; z^4, the same at four times for QPSK.  fsea_plan transforms one contiguous buffer at one
 * hop and writes a row per frame; an event list is hundreds of scattered spans of different lengths that each want one
 * averaged row.  An fsea_spectra holds the transform size n (a power of two in [FSEA_SPECTRA_MIN_N, FSEA_SPECTRA_MAX_N]),
 * the hop in [1, n], the kind and an optional taper w of n finite f32 weights (NULL: rectangular), takes a table of jobs
 * over one resident buffer of f32 pairs and writes n f32 powers per job at power + out_first.  There is no state between
 * calls and no reset.
 *   terms:      for pair i of a job, z_i = pairs[first_pair + i] (rn = one IEEE rounding, round to nearest even; nothing is
 *               contracted into an FMA):
 *                 a_i = (float) rn((double)re_i - offset_re),   b_i = (float) rn((double)im_i - offset_im)
 *               (the subtraction in f64, then the conversion's rounding); offset is the pedestal the caller knows,
 *               (0.5 + 0.5j) sum(c) of the extract's taps, as for the measures.  From there on everything is f32.
 *   kinds:      FSEA_SPECTRA_Z:        (u, v) = (a, b)
 *               FSEA_SPECTRA_ENVELOPE: u = rn(rn(a a) + rn(b b)),  v = +0.0
 *               FSEA_SPECTRA_SQUARE:   u = rn(rn(a a) - rn(b b)),  v = rn(2 rn(a b))
 *               FSEA_SPECTRA_FOURTH:   SQUARE applied to SQUARE's (u, v)
 *   segments:   S = n_pairs < n ? 0 : (n_pairs - n) / hop + 1 (rounded down).  Segment s covers pairs s hop .. s hop + n - 1
 *               of the job; its input is x_j = (-1)^j (rn(w_j u), rn(w_j v)), j = 0 .. n - 1.  Without a taper there is no
 *               multiplication; a taper of all 1.0f gives the bits of NULL.
 *   transform:  X_s[k] = sum over j of x_j e^(-2 pi i j k / n) in f32: a radix-4 Stockham transform (a last radix-2 pass where
 *               log2 n is odd) with twiddles rounded to f32 from f64; its roundings are the implementation's.  With the sign
 *               (-1)^j bin k is the frequency (k - n / 2) / n cycles per pair: the cut-out's centre is bin n / 2, as
 *               everywhere in this library.  p_s[k] = rn(rn(re^2) + rn(im^2)) in f32.
 *   average:    the f32 p_s[k] are widened to f64 and added in segment order: a job's segments are cut into tiles of
 *               FSEA_SPECTRA_TILE_SEGMENTS counted from the job's own segment 0; a tile's partial starts at +0.0 and adds
 *               its segments ascending; a job's sum adds the tiles' partials ascending;
 *                 power[out_first + k] = (float) rn(sum / (double)S).
 *               Nothing in this depends on first_pair (at any parity), on the other jobs, on their order or on the launch
 *               geometry: a job's n floats are the same bits alone or in a table of FSEA_SPECTRA_MAX_JOBS.  A NaN or an
 *               infinity in one job's pairs shows in that job's output alone.
 *   table:      jobs may overlap and may repeat in the input; their output ranges must not overlap and lie inside n_power.
 *               A job with S = 0 (an empty one too) has no output, writes nothing and is legal.  Only the jobs' pairs are
 *               read, only the jobs' outputs are written.  `jobs` is host memory, read before the call returns.
 *   create:     FSEA_EINVAL, in this order, for a NULL out-pointer, an n that is not a power of two in [64, 4096], a hop
 *               outside [1, n], an unknown kind, a window weight that is not finite; only then FSEA_ENODEVICE without a
 *               GPU.  The window is copied.  n and hop return 0 for NULL, kind -1.  Destroy waits for the device.
 *   segments:   S for a span of n_pairs; 0 for a NULL object.
 *   layout:     fills out_first back to back in table order -- every job with S > 0 gets n floats, a job with S = 0 the
 *               running position and none -- and gives the floats needed in *total_floats.  FSEA_EINVAL for a NULL object or
 *               total_floats, n_jobs above FSEA_SPECTRA_MAX_JOBS, a NULL table with n_jobs > 0.
 *   run_device: d_pairs (n_buffer_pairs pairs of floats) 8-byte aligned, d_power (n_power floats) 4-byte aligned;
 *               asynchronous on `stream`.  The object owns the device copy of the table and the tiles' partials and grows
 *               them as needed, so calls on several streams follow one another (an event).  Kernel fsea_spectra_tiles_<n>:
 *               one workgroup per tile of one job, which it finds by a bisection over the jobs' first tiles; kernel
 *               fsea_spectra_fold: the tiles' partials in order, the division, the store.
 *   run_host:   the same from and to host memory through pinned staging on the object's own stream; returns when `power` is
 *               complete; of `power` only the jobs' output ranges are written.
 * Both check, before any device work and reading nothing of the object but n and hop, in this order: a NULL object; n_jobs
 * above FSEA_SPECTRA_MAX_JOBS; n_jobs == 0 is then a successful no-op; a NULL job table; a NULL buffer (pairs or power); an
 * offset that is not finite; per job in table order: first_pair + n_pairs past n_buffer_pairs, n_pairs above
 * FSEA_SPECTRA_MAX_PAIRS, for a job with output out_first + n past n_power (each text names the job); two output ranges that
 * overlap (the text names both jobs); more than 2^31 transformed points (the sum of S n) in the call; for run_device a
 * d_pairs that is not 8-byte or a d_power that is not 4-byte aligned.  All FSEA_EINVAL; a refused call writes nothing.  Calls
 * on one object from several threads are serialised.
 *   jobs:       fsea_spectra_jobs, host arithmetic, no device: the twin of fsea_measure_jobs -- the spans of the outputs of
 *               extract jobs that were laid out, without the first skip_pairs of each; out_first is set to 0
 *               (fsea_spectra_layout places them).  The same refusals, the cap FSEA_SPECTRA_MAX_PAIRS.
 *   finish:     fsea_spectra_finish, host arithmetic, callable in a process without a GPU: one row P of n powers to its
 *               figures, all in f64, every sum over k ascending:
 *                 total             = sum P[k]
 *                 centroid_cycles   = sum (k - n/2) P[k] / total / n
 *                 the occupied band at `fraction` (0.99, say): t = total (1 - fraction) / 2, c[k] the running sum;
 *                 obw_lo            = the least k with c[k] > t;   obw_hi = the least k with c[k] >= total - t
 *                 obw_bins          = obw_hi - obw_lo + 1;   obw_centre_cycles = ((obw_lo + obw_hi) / 2 - n/2) / n
 *                 the strongest line, among the bins outside |k - n/2| <= guard_bins (guard_bins = -1 guards nothing):
 *                 peak_bin          = the lowest k with the maximum;  peak_power = P[peak_bin];
 *                 peak_cycles       = (peak_bin - n/2) / n
 *                 floor             = the lower median of the same bins (element (m - 1) / 2 of the m, ascending)
 *                 line_db           = 10 log10(peak_power / floor)
 *               With total == 0 the ratios are NaN, there is no band (obw_lo = obw_hi = -1, obw_bins = 0, obw_centre_cycles
 *               NaN) and the call still returns FSEA_OK; so with a NaN among the powers.  FSEA_EINVAL, in this order, for a
 *               NULL pointer, an n that is not a power of two in [64, 4096], guard_bins outside [-1, n/2 - 1], fraction
 *               outside (0, 1]. */
#define FSEA_SPECTRA_Z        0
#define FSEA_SPECTRA_ENVELOPE 1
#define FSEA_SPECTRA_SQUARE   2
#define FSEA_SPECTRA_FOURTH   3
#define FSEA_SPECTRA_MIN_N    64
#define FSEA_SPECTRA_MAX_N    4096
#define FSEA_SPECTRA_TILE_SEGMENTS 32
#define FSEA_SPECTRA_MAX_JOBS  65536        /* = FSEA_EXTRACT_MAX_JOBS */
#define FSEA_SPECTRA_MAX_PAIRS (1u << 24)   /* per job */
typedef struct { uint64_t first_pair, n_pairs, out_first; } fsea_spectra_job;   /* 24 bytes */
typedef struct {                                                                 /* 72 bytes */
    double total, centroid_cycles, obw_centre_cycles;
    double peak_power, peak_cycles, floor, line_db;
    int32_t obw_lo, obw_hi, obw_bins, peak_bin;
} fsea_spectra_result;
typedef struct fsea_spectra fsea_spectra;
int fsea_spectra_create(fsea_spectra **spectra, int n, int hop, int kind, const float *window, int device);
int fsea_spectra_destroy(fsea_spectra *spectra);
int fsea_spectra_n(const fsea_spectra *spectra);
int fsea_spectra_hop(const fsea_spectra *spectra);
int fsea_spectra_kind(const fsea_spectra *spectra);
size_t fsea_spectra_segments(const fsea_spectra *spectra, size_t n_pairs);
int fsea_spectra_layout(const fsea_spectra *spectra, fsea_spectra_job *jobs, size_t n_jobs, size_t *total_floats);
int fsea_spectra_run_device(fsea_spectra *spectra, const void *d_pairs, size_t n_buffer_pairs, const fsea_spectra_job *jobs,
                            size_t n_jobs, double offset_re, double offset_im, float *d_power, size_t n_power, void *stream);
int fsea_spectra_run_host(fsea_spectra *spectra, const float *pairs, size_t n_buffer_pairs, const fsea_spectra_job *jobs,
                          size_t n_jobs, double offset_re, double offset_im, float *power, size_t n_power);
int fsea_spectra_jobs(const fsea_extract_job *ejobs, size_t n_jobs, int decimation, size_t skip_pairs, fsea_spectra_job *jobs);
int fsea_spectra_finish(const float *power, int n, int guard_bins, double fraction, fsea_spectra_result *result);

/* The burst detector of the reference's signal scene (lua/signal-detector.lua:93-96): nrf_signal_detector_process
 * (src/nrf.c:883-898) on n_blocks consecutive blocks of block_bytes 8-bit samples behind one pointer.  With
 * x_i = byte_i / 256.0 and n = block_bytes the reference computes
 *     mean = (sum of x_i over even i) / n * 2,    standard_deviation = sqrt(sum over all i of (x_i - mean)^2 / mean)
 * -- it divides by the mean, not by n; an all-zero block gives NaN.  The device part is three exact unsigned 64-bit sums per
 * block over the bytes as the detector sees them (flip != 0: b ^ 0x80 first, as in the other entry points): sums[3 b] the
 * bytes at even offsets of block b, sums[3 b + 1] all bytes, sums[3 b + 2] their squares.  Integer sums: the same bits
 * whatever the launch geometry, one launch of n_blocks blocks or n_blocks launches of one.
 *   u8_device: asynchronous on `stream`; d_iq and d_sums 16-byte aligned; only the n_blocks * block_bytes bytes are read.
 *   u8_host:   upload, launch, finish: mean[b] and sd[b] per block.  Staged through pinned memory on the object's own
 *              stream; calls on one object from several threads are serialised.
 *   moments, finish: host arithmetic, callable in a process without a GPU.  mean is the reference's value bit for bit (its
 *              first loop adds multiples of 1/256 below 2^53: exact).  diffs_total, the reference's sum of (x_i - mean)^2,
 *              comes from the sums centred on the integer nearest to 256 mean in exact 64-bit arithmetic, so a quiet block
 *              loses nothing to cancellation (within 8 * 2^-53 relative of the exact value, exactly 0 where that is 0);
 *              sd = sqrt(diffs_total / mean) with the reference's division and root, NaN for a zero mean.
 * Every form checks its arguments before any device work: FSEA_EINVAL for a NULL object or buffer, a block_bytes that is
 * odd, below 2 or above 2^31, n_blocks == 0, more than 2^40 bytes in all, a misaligned device pointer, sums no block of
 * n_elements bytes can have.  Create: FSEA_ENODEVICE without a GPU.  Destroy waits for the device. */
int fsea_detect_create(fsea_detect **detect, int device);
int fsea_detect_destroy(fsea_detect *detect);
int fsea_detect_u8_device(fsea_detect *detect, const void *d_iq, size_t block_bytes, size_t n_blocks, int flip,
                          uint64_t *d_sums, void *stream);
int fsea_detect_u8_host(fsea_detect *detect, const uint8_t *iq, size_t block_bytes, size_t n_blocks, int flip, double *mean,
                        double *sd);
int fsea_detect_moments(const uint64_t sums[3], size_t n_elements, double *mean, double *diffs_total);
int fsea_detect_finish(const uint64_t sums[3], size_t n_elements, double *mean, double *sd);

/* The signal scene on a recording that stays on the device (lua/signal-detector.lua:89-133): detect the bursts, low-pass
 * the blocks of each burst, keep them appended, draw a burst as a growing line image.  The object owns a detector
 * (fsea_detect), a chain (fsea_chain: the filter taps are given at create, the stream's tail is carried), a draw object and
 * a growing device buffer of the bursts' filtered f32 pairs.  Nothing here computes beyond the detector: the filter launches
 * are fsea_chain_run_device on runs of consecutive blocks of the resident recording and the images are
 * fsea_iq_lines_device (FSEA_IQ_F32) on a resident burst, so every pair and every pixel is what those calls give, bit for
 * bit.
 *   scan: one detector launch over all blocks, one copy of 24 n_blocks bytes to the host, the scene's state machine there
 *       (fsea_capture_segment), then per burst one filter run over its blocks, n_frames = its block count, appended to the
 *       burst buffer: what nut_buffer_append builds in the scene's draw_buffer.  Returns when the bursts are complete.
 *       The filter's tail carries across bursts and across scans, and so does the state machine: a burst still open at the
 *       end of a scan is reported with open != 0 and continued by the next scan.  Bursts accumulate, numbered from 0, until
 *       reset, which also zeroes the tail.  block_bytes is a multiple of 16 here (every run of blocks is then a 16-byte
 *       aligned piece of the recording); d_iq 16-byte aligned.  scan_host uploads the recording into device memory of the
 *       object first.
 *       A scan that fails after the detector (a filter launch, an allocation) leaves the bursts, the statistics and the
 *       filter's tail partly advanced: call reset before the object is used again.
 *   segment: the state machine alone, host arithmetic.  DETECTING: a block with sd > threshold starts a burst.  CAPTURING:
 *       blocks with sd > threshold join it; the first block at or below the threshold ends it and is dropped.  A NaN is
 *       not above the threshold.  capturing != 0: a burst is open from an earlier scan; runs[0] then continues it
 *       (continues != 0) and may have no block at all, when the first block ends it.  `runs` has room for
 *       n_blocks / 2 + 1 entries.
 *   stats: mean and standard deviation of block `block` of the last scan.
 *   burst: first_block counts the blocks of all scans since create or reset; d_pairs is valid until the next scan, reset
 *       or destroy.  burst_pairs_host: 2 n_pairs floats.  burst_lines_*: fsea_iq_lines_* over the burst's first
 *       n_line_points pairs; the device form is asynchronous on `stream`, d_image 16-byte aligned.
 * Every form checks its arguments before any device work (FSEA_EINVAL: as fsea_detect_u8_device, a block_bytes that is no
 * multiple of 16, a block or burst index out of range, n_line_points above the burst's pairs, a size_multiplier outside
 * [1, FSEA_IQ_MAX_MULTIPLIER]).  Create: as fsea_fir_create, FSEA_ENODEVICE without a GPU.  Destroy and reset wait for the
 * device.  Calls on one object from several threads are serialised. */
typedef struct {
    size_t first_block;   /* in the scan's blocks (fsea_capture_segment) or in all blocks since reset (fsea_capture_burst) */
    size_t n_blocks;
    int continues;        /* the run belongs to the burst that was open before the scan */
    int open;             /* the scan ended inside the run */
} fsea_capture_run;

typedef struct {
    size_t first_block;
    size_t n_blocks;
    size_t n_pairs;
    int open;
    const float *d_pairs; /* device memory: n_pairs (I, Q) pairs */
} fsea_capture_burst_info;

int fsea_capture_create(fsea_capture **capture, const double *taps, int n_taps, int device);
int fsea_capture_destroy(fsea_capture *capture);
int fsea_capture_reset(fsea_capture *capture);
int fsea_capture_scan_device(fsea_capture *capture, const void *d_iq, size_t block_bytes, size_t n_blocks, int flip,
                             double threshold, void *stream);
int fsea_capture_scan_host(fsea_capture *capture, const uint8_t *iq, size_t block_bytes, size_t n_blocks, int flip,
                           double threshold);
int fsea_capture_segment(const double *sd, size_t n_blocks, double threshold, int capturing, fsea_capture_run *runs,
                         size_t *n_runs);
size_t fsea_capture_n_blocks(const fsea_capture *capture);
int fsea_capture_stats(const fsea_capture *capture, size_t block, double *mean, double *sd);
size_t fsea_capture_n_bursts(const fsea_capture *capture);
int fsea_capture_burst(const fsea_capture *capture, size_t burst, fsea_capture_burst_info *info);
int fsea_capture_burst_pairs_host(fsea_capture *capture, size_t burst, float *pairs);
int fsea_capture_burst_lines_device(fsea_capture *capture, size_t burst, int size_multiplier, size_t n_line_points,
                                    void *d_image, void *stream);
int fsea_capture_burst_lines_host(fsea_capture *capture, size_t burst, int size_multiplier, size_t n_line_points,
                                  uint8_t *image);

/* Blends of two resident sample blocks for an array of weights: the batched form of the reference's nrf_interpolator
 * (src/nrf.c:442-496) and of the frame loop of its movie tool (c/gradual-noise.c:96-112).  The object owns two device
 * blocks A and B of n_elements elements of one type, FSEA_IQ_U8 or FSEA_IQ_F64, zero after create and reset.
 *   push:   A takes what B held, B takes the new block.  Only the new block is copied; A and B change roles by pointer.
 *   frames: frame f, element i is the reference's nrf_interpolator_get_buffer loop with t = weights[f]:
 *           v = a (1.0 - t) + b t in double, two products and one sum, each rounded (no fused multiply-add).  F64 blocks:
 *           a, b and the output are the doubles themselves.  U8 blocks: a and b are byte / 256.0 and the output byte is
 *           x86-64's (uint8_t)(v * 256.0) as for the IQ images above (so a NaN weight gives 0).  The weights are doubles
 *           of any value; the reference's own t ends each ramp a little above 1.  Frame f is the f-th n_elements
 *           elements of the output.
 *   image_frames (U8 blocks of at least 2 iq_size^2 bytes): frame f is a width x height u8 image, the tool's frame for
 *           the weight w = weights[f], which arrives already eased.  Sample (x, y) of the iq_size x iq_size grid is byte
 *           2 (y iq_size + x) of the blocks (flip != 0: b ^ 0x80 first, the tool's (b + 128) % 256) as an integer 0...255;
 *           pwr = a (1.0 - w) + b w in double as above, colour = (int) of pwr clamped to [0, 255] (0 for a NaN).  Pixel
 *           (px, py) takes the colour of sample (col[px], row[py]): the last sample, in the tool's raster order, whose
 *           put_block covers it, with BLOCK_SCALE = max(width, height) / (double) iq_size.  fsea_interp_image_tables gives
 *           the two tables (host arithmetic, the tool's loops in one dimension each; needs no device).
 * Device forms: asynchronous on `stream`; weights, blocks and outputs are device memory, outputs 16-byte and weights 8-byte
 * aligned.  Calls on one object take effect in stream order (a push is seen by the frames queued behind it on that
 * stream); across streams the caller orders them.  The first image call with a new geometry uploads its tables and
 * waits for the object's earlier image launches.
 * Host forms return when the output is complete (a push: when the block is on the device); staged through pinned memory
 * on the object's own stream, calls on one object from several threads are serialised.
 * Every form checks its arguments before any device work: FSEA_EINVAL for a NULL object or buffer, a type other than the
 * two, more than 2^31 elements, n_frames < 0, a misaligned device buffer, a width or height outside [1, 16384], an
 * iq_size outside [1, 4096], blocks that are not U8 or too short for the image form.  n_frames == 0 writes nothing.
 * Create: FSEA_ENODEVICE without a GPU.  Destroy and reset wait for the device. */
typedef struct {
    int width, height; /* of one image */
    int iq_size;       /* the sample grid is iq_size x iq_size */
    int flip;          /* != 0: raw HackRF int8 bytes */
} fsea_interp_geometry;

int fsea_interp_create(fsea_interp **interp, int type, size_t n_elements, int device);
int fsea_interp_destroy(fsea_interp *interp);
int fsea_interp_reset(fsea_interp *interp);
size_t fsea_interp_n_elements(const fsea_interp *interp);
int fsea_interp_push_device(fsea_interp *interp, const void *d_block, void *stream);
int fsea_interp_push_host(fsea_interp *interp, const void *block);
int fsea_interp_frames_device(fsea_interp *interp, const double *d_weights, int n_frames, void *d_out, void *stream);
int fsea_interp_frames_host(fsea_interp *interp, const double *weights, int n_frames, void *out);
/* col: width entries, row: height entries; entry p is the sample whose colour pixel column / row p shows. */
int fsea_interp_image_tables(int width, int height, int iq_size, int32_t *col, int32_t *row);
int fsea_interp_image_frames_device(fsea_interp *interp, const double *d_weights, int n_frames,
                                    const fsea_interp_geometry *geometry, void *d_images, void *stream);
int fsea_interp_image_frames_host(fsea_interp *interp, const double *weights, int n_frames,
                                  const fsea_interp_geometry *geometry, uint8_t *images);

/* The IQ trace movie: the frame loop of the reference's c/single-sample.c ("slowly show a single sample, frame by frame")
 * on a canvas that stays on the device.  The object owns a width x height u8 canvas, zero after create and reset, with the
 * (256 m) x (256 m) IQ square at OX = (width - 256 m) / 2, OY = (height - 256 m) / 2, m = size_multiplier.
 *   frames: frame f of a call takes the bytes from f * frame_bytes on.  Its points are P[k] = (b[2k], b[2k + 1]) for
 *           2k < frame_bytes (flip != 0: b ^ 0x80 first, the tool's (b + 128) % 256), as far as both bytes of a point lie
 *           inside the n_bytes readable bytes of the call: with an odd frame_bytes the Q byte of a frame's last point is the
 *           first byte of the next frame, as in the tool, and a caller whose data goes on passes at least
 *           n_frames * frame_bytes + 1 bytes; where the data ends earlier the rest of the frame is not drawn (the tool
 *           reads past its buffer there), and a frame wholly behind the data only fades.
 *           1. every canvas pixel v becomes max(v - fade, 0);
 *           2. the reference's draw_line (as fsea_iq_lines_*) runs from m P[k-1] to m P[k] for k >= 1; the last point of
 *              the previous frame is not joined to P[0].  A hit on (x, y) is skipped when x == 0, y == 0, x == width - 1 or
 *              y == height - 1 (the tool compares IQ-square coordinates with the canvas size); otherwise canvas pixel
 *              (x + OX, y + OY), of value v, becomes v + pixel_inc unless v + pixel_inc >= 255;
 *           3. the canvas is image f of the output (width x height bytes, rows top to bottom).
 *           d_images / images NULL: the canvas advances and no frame is written (the tool's -v).
 * The frames are exact: h hits of a frame on a pixel of faded value v leave v + pixel_inc min(h, (254 - v) / pixel_inc),
 * whatever their order.  The same bytes fed in one call or in calls of any numbers of frames give the same frames and the
 * same canvas.
 * Device form: asynchronous on `stream`; d_images 16-byte aligned.  The canvas and the count planes are the object's: its
 * calls on several streams follow one another on the device (each waits for an event the previous one recorded).
 * Host forms return when the output is complete; staged through pinned memory on the object's own stream, calls on one
 * object from several threads are serialised.  canvas_host: the canvas as it stands after the calls made so far.
 * Every form checks its arguments before any device work: FSEA_EINVAL for a NULL object, config or buffer, 256 m above the
 * width or the height, a width or height above 16384, an m outside [1, FSEA_IQ_MAX_MULTIPLIER], a pixel_inc outside
 * [1, 254], a fade outside [0, 255], frame_bytes == 0 or above 2^31, n_frames < 0, a misaligned d_images.  n_frames == 0
 * does nothing.  Create: FSEA_ENODEVICE without a GPU.  Destroy and reset wait for the device. */
typedef struct {
    int width, height;   /* of the canvas and of every frame */
    int size_multiplier; /* the IQ square is 256 m x 256 m */
    int pixel_inc;       /* the tool's -p */
    int fade;            /* the tool's -f, per frame */
} fsea_trace_config;

int fsea_trace_create(fsea_trace **trace, const fsea_trace_config *config, int device);
int fsea_trace_destroy(fsea_trace *trace);
int fsea_trace_reset(fsea_trace *trace);
int fsea_trace_frames_device(fsea_trace *trace, const void *d_bytes, size_t n_bytes, int flip, size_t frame_bytes,
                             int n_frames, uint8_t *d_images, void *stream);
int fsea_trace_frames_host(fsea_trace *trace, const void *bytes, size_t n_bytes, int flip, size_t frame_bytes, int n_frames,
                           uint8_t *images);
int fsea_trace_canvas_host(fsea_trace *trace, uint8_t *image);

/* The reference's audio chain (src/nrf.c:778-1094: nrf_downsampler, nrf_raw_demodulator, nrf_fm_demodulator,
 * nrf_decoder) as a streaming decoder of n_channels channels over one input stream, each channel with its own frequency
 * offset, phase and state.  f64 arithmetic on the device.  Per call on n input samples, channel ch:
 *   x[k] = (c + i s) e^{i theta k} (I[k], Q[k]),  theta = 2 pi freq_offset / in_rate, the phase of sample k taken from the
 *          exactly reduced cycle count (freq_offset k mod in_rate) / in_rate; u8 input: I = b[2k] / 128.0 - 0.995 (the
 *          reference's decoder conversion; flip != 0: raw HackRF int8 bytes, b ^ 0x80 first), f64 input as is
 *   RAW:   audio = the reference's downsampler (in_rate -> out_rate, cutoff out_rate / 2, 41 taps) on I
 *   WBFM:  downsamplers (in_rate -> 336000, cutoff 60000, 51 taps) on I and Q, the reference's discriminator with the
 *          previous stage-1 output carried across calls (0 after create and reset), a downsampler (336000 -> out_rate,
 *          cutoff 10000, 41 taps), de-emphasis v += alpha (x - v), alpha = 1 / (1 + out_rate 50e-6), v carried
 * A downsampler keeps the last L - 1 inputs across calls and computes output j of a call at x_ext[idx_j ..], idx_j the
 * reference's accumulated floor(t), t += in / (double) out from 0 on every call; out_length = floor(n / rate_mul).  The
 * index tables are built on the host by that accumulation and cached per call length.
 * Channel ch of a K-channel object gives bit for bit what a 1-channel object with the same offset and phase gives.
 * Errors: every form checks its arguments before any device work (FSEA_EINVAL: NULL object or buffer, unknown type,
 * rates <= 0, n_channels outside [1, FSEA_DEMOD_MAX_CHANNELS], n_samples above FSEA_DEMOD_MAX_SAMPLES or giving more than
 * FSEA_DEMOD_MAX_SAMPLES outputs of a stage, a channel out of range, a non-finite phase).  Create: FSEA_ENODEVICE without a
 * GPU.  Destroy waits for the device. */
enum { FSEA_DEMOD_RAW = 0, FSEA_DEMOD_WBFM = 1 };   /* = nrf_demodulate_type values */
#define FSEA_DEMOD_MAX_CHANNELS 256
#define FSEA_DEMOD_MAX_SAMPLES (1 << 24)

int fsea_demod_create(fsea_demod **demod, int type, int in_rate, int out_rate, int n_channels, int device);
int fsea_demod_destroy(fsea_demod *demod);
/* Tails, carried stage-1 outputs and de-emphasis values to 0, every phase to (1, 0); offsets stay.  Waits for the device. */
int fsea_demod_reset(fsea_demod *demod);
/* The offset and phase (cosine, sine) channel ch starts its next call with; get returns them, after a call advanced by
 * theta n with the same reduction (host arithmetic). */
int fsea_demod_set_channel(fsea_demod *demod, int ch, int freq_offset, double cosine, double sine);
int fsea_demod_get_channel(const fsea_demod *demod, int ch, int *freq_offset, double *cosine, double *sine);
/* Audio samples per channel of a call on n_samples (0 for a NULL object or an n_samples the object rejects). */
size_t fsea_demod_out_length(const fsea_demod *demod, size_t n_samples);
/* Device form: d_iq holds 2 * n_samples bytes (2-byte aligned), d_audio receives n_channels rows of out_length f64,
 * row-major (8-byte aligned).  Asynchronous on `stream`; successive calls on one stream continue one signal, across
 * streams the caller orders them. */
int fsea_demod_u8_device(fsea_demod *demod, const void *d_iq, size_t n_samples, int flip, double *d_audio, void *stream);
/* Host forms; return when `audio` is complete.  Staged through pinned memory on the object's own stream; calls on one
 * object from several threads are serialised.  The f64 form takes separate I and Q arrays and converts nothing. */
int fsea_demod_u8_host(fsea_demod *demod, const uint8_t *iq, size_t n_samples, int flip, double *audio);
int fsea_demod_f64_host(fsea_demod *demod, const double *i, const double *q, size_t n_samples, double *audio);

const char *fsea_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif
