/*
 * fsea-cutouts -- from a recording to one IQ file per emission: fsea-events finds the time-frequency boxes, this tool turns
 * each box back into its signal, mixed to the centre, low-passed and decimated by D.
 *
 * Pass 1 is fsea-events' for a recording: every frame of N samples (one every H) through a plan in a dB mode, the rows to a
 * fsea_cfar object with a mask, mask and rows to a fsea_events object, all on the device chunk by chunk; the runs are kept
 * on the host and linked once at the end (tool_common.h); --axis time|either: fsea-events', the detector down the time axis
 * alone or OR-ed into that mask.  Pass 2 turns the first --max-events surviving events into jobs with
 * fsea_extract_jobs (include/fsea.h): a job begins fsea_extract_lead samples in front of its box, so that the filter has run
 * in where the box begins, and ends with the last frame of the box; a job longer than --max-samples is cut short.  The jobs
 * are grouped into batches whose samples total at most 64 MiB; the byte ranges of a batch are read from the file into one
 * pinned buffer back to back, every job's `first` rebased to its place there (sample_offset stays the stream position), and
 * the batch is uploaded and run in one fsea_extract_run_device call.  Cut-out j is written as DIR/cutout-%05u.cf32: raw
 * little-endian f32 pairs at RATE / D, without the first lead / D outputs (the filter's run-in).  DIR/cutouts.txt gets one
 * line per event:
 *     number row_first row_last col_first col_last first_sample samples centre_mhz output_rate pairs fits cut_short
 * (centre_mhz and output_rate are 0 without --rate and --freq).  An event whose columns times D exceed --fill of the N
 * columns does not fit the decimated band and gets no file (fits 0); neither does one past --max-events or one with no
 * output behind the run-in.  The tool prints
 *     rows R runs N events E cutouts C skipped S
 *
 * --measures, --audio fm|am and --spectra N: the three stages below, each on a batch's pairs while they are resident.  The
 * options: USAGE.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>

#include "fsea.h"
#include "tool_common.h"

#define TOOL "fsea-cutouts"
#define BATCH_SAMPLES ((size_t)32 << 20) /* 64 MiB of 8-bit IQ */

static const char *USAGE =
    "usage: fsea-cutouts FILE --size N --decimation D --out DIR [--hop H] [--window NAME] [--flip] [--mode db5|db10|db]\n"
    "                    [--guard G] [--train T] [--offset LEVELS] [--method ca|go|so] [--rank R] [--axis freq|time|either]\n"
    "                    [--gap-cols B] [--gap-rows R] [--min-rows R] [--min-cols B] [--min-hits K] [--rate HZ --freq MHZ]\n"
    "                    [--taps L] [--cutoff HZ]\n"
    "                    [--fill F] [--max-events E] [--max-samples S] [--measures [--lag K]]\n"
    "                    [--audio fm|am [--audio-rate HZ] [--audio-taps N] [--audio-cutoff HZ] [--deviation HZ]]\n"
    "                    [--spectra N [--spectra-hop H] [--spectra-kind z|env|sq|fourth] [--spectra-window NAME]\n"
    "                     [--spectra-guard G] [--spectra-fraction F]]\n"
    "  FILE is a raw 8-bit IQ recording (--flip: HackRF int8).  The emissions are found as fsea-events finds them (its\n"
    "  options, same defaults); each one whose columns times D fill at most F of the N columns is mixed to the centre,\n"
    "  low-passed (L taps, half amplitude at --cutoff, default 0.4 RATE / D) and decimated by D on the GPU, all of a batch in\n"
    "  one launch, and written to DIR/cutout-NNNNN.cf32 as f32 pairs; DIR/cutouts.txt lists every event.  A cut-out longer\n"
    "  than S samples is cut short.  --measures: DIR/measures.txt says of every cut-out written its power in dB, its\n"
    "  frequency offset (lag K pairs, default 1), spectrum width, envelope kurtosis, crest factor and what is left of its DC.\n"
    "  --audio: every cut-out written is FM- or AM-demodulated on the GPU, low-passed (N taps, half amplitude at\n"
    "  --audio-cutoff, default 0.4 of the audio rate) and decimated to about --audio-rate; DIR/cutout-NNNNN.wav is mono 16-bit\n"
    "  PCM, full scale at --deviation for FM, and DIR/audio.txt lists number, rate, samples and peak of every file.  Needs --rate.\n"
    "  --spectra: the averaged periodogram of every cut-out written, N bins (a power of two in [64, 4096]) every H pairs\n"
    "  (default N / 2) under the taper NAME (--window's names, default hann), on the GPU: of the cut-out itself (z), of its\n"
    "  envelope |z|^2 (env: a line at the symbol rate), of z^2 (sq: a line at twice a BPSK carrier's offset) or of z^4\n"
    "  (fourth: four times a QPSK carrier's).  DIR/spectra.txt lists number, segments, the bandwidth that holds F of the\n"
    "  power (default 0.99), the centroid and the strongest line outside G bins round the centre (default 0 for z, 2\n"
    "  otherwise; -1: none) -- in Hz with --rate, in cycles per pair without -- and the line's height over the median in dB.\n"
    "  Prints `rows R runs N events E cutouts C skipped S`, with --audio followed by ` audio A`, with --spectra by ` spectra P`\n"
    "  defaults: --taps 97 --fill 0.8 --max-events 1024 --max-samples 16777216 --audio-rate 48000 --audio-taps 41 --deviation 75000";

static void usage_error(const char *msg) { tool_usage_error(TOOL, msg); }

static void die(const char *what) { tool_die(TOOL, what); }

/* 16 and 32 bits, little-endian */
static void put_le(uint8_t *at, uint32_t value, int bytes) {
    for (int i = 0; i < bytes; i++) at[i] = (uint8_t)(value >> (8 * i));
}

/* DIR/cutout-NNNNN.wav: the 44-byte header of mono 16-bit PCM, n samples of audio - mean, *peak their largest; 0: written */
static int write_wav(FILE *out, uint32_t rate, const float *audio, double mean, size_t n, double *peak) {
    uint8_t head[44];
    memcpy(head, "RIFF", 4);
    put_le(head + 4, (uint32_t)(36 + 2 * n), 4);
    memcpy(head + 8, "WAVEfmt ", 8);
    put_le(head + 16, 16, 4);
    put_le(head + 20, 1, 2);        /* PCM */
    put_le(head + 22, 1, 2);        /* one channel */
    put_le(head + 24, rate, 4);
    put_le(head + 28, 2 * rate, 4); /* bytes a second */
    put_le(head + 32, 2, 2);        /* bytes a sample */
    put_le(head + 34, 16, 2);
    memcpy(head + 36, "data", 4);
    put_le(head + 40, (uint32_t)(2 * n), 4);
    int bad = fwrite(head, 1, sizeof(head), out) != sizeof(head);
    *peak = 0.0;
    for (size_t i = 0; i < n && !bad; i++) {
        const double v = (double)audio[i] - mean, s = v * 32000.0, mag = v < 0.0 ? -v : v;
        const int16_t pcm = s >= 32767.0 ? 32767 : s <= -32768.0 ? -32768 : s == s ? (int16_t)s : 0;
        uint8_t two[2];
        if (mag > *peak) *peak = mag;
        put_le(two, (uint16_t)pcm, 2);
        bad = fwrite(two, 1, 2, out) != 2;
    }
    return bad;
}

/* Room for DIR/<any name of the output>: main's, after the checks.  Below, `format` makes the name of DIR and a number. */
static char *out_name;
static size_t out_name_len;

/* a file of the output that could not be written: the one named last */
static void cannot_write(void) {
    fprintf(stderr, TOOL ": cannot write %s\n", out_name);
    exit(EXIT_FAILURE);
}

/* DIR/<name> open for writing, or the tool ends */
static FILE *open_in(const char *dir, const char *format, unsigned number, const char *mode) {
    snprintf(out_name, out_name_len, format, dir, number);
    FILE *f = fopen(out_name, mode);
    if (f == NULL) cannot_write();
    return f;
}

/* DIR/<name> closed and, with `bad` 0, written whole, or the tool ends */
static void close_in(FILE *f, int bad, const char *dir, const char *format, unsigned number) {
    snprintf(out_name, out_name_len, format, dir, number);
    if ((fclose(f) != 0) | bad) cannot_write();
}

typedef struct {
    const char *path, *out_dir, *window, *mode_name, *audio_name, *spectra_kind_name, *spectra_window;
    int size, hop, flip, gap_cols, gap_rows, decimation, n_taps, measures, lag, audio_taps;
    int spectra, spectra_hop, spectra_guard, spectra_guard_given, spectra_sub; /* spectra 0: no --spectra; _sub: a --spectra-* was given */
    long long min_rows, min_cols, min_hits, max_events, max_samples;
    double cutoff, fill, audio_rate, audio_cutoff, deviation, spectra_fraction;
    tool_detector det;
    int mode, type, audio_kind, audio_decimation; /* what the checks make of the names and rates; audio_kind -1: no --audio */
    int spectra_kind, spectra_window_kind;
} options;

/* the command line into *o (the defaults are the caller's), every value checked: a wrong one ends the tool */
static void parse_options(int argc, char **argv, options *o) {
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--help")) {
            puts(USAGE);
            exit(0);
        } else if (!strcmp(argv[i], "--size") && more) o->size = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--hop") && more) o->hop = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--window") && more) o->window = argv[++i];
        else if (!strcmp(argv[i], "--flip")) o->flip = 1;
        else if (!strcmp(argv[i], "--mode") && more) o->mode_name = argv[++i];
        else if (tool_detector_option(TOOL, &o->det, argc, argv, &i)) continue;
        else if (!strcmp(argv[i], "--gap-cols") && more) o->gap_cols = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gap-rows") && more) o->gap_rows = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--min-rows") && more) o->min_rows = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-cols") && more) o->min_cols = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-hits") && more) o->min_hits = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--decimation") && more) o->decimation = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--taps") && more) o->n_taps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--cutoff") && more) o->cutoff = atof(argv[++i]);
        else if (!strcmp(argv[i], "--fill") && more) o->fill = atof(argv[++i]);
        else if (!strcmp(argv[i], "--max-events") && more) o->max_events = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--max-samples") && more) o->max_samples = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--measures")) o->measures = 1;
        else if (!strcmp(argv[i], "--lag") && more) o->lag = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--audio") && more) o->audio_name = argv[++i];
        else if (!strcmp(argv[i], "--audio-rate") && more) o->audio_rate = atof(argv[++i]);
        else if (!strcmp(argv[i], "--audio-taps") && more) o->audio_taps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--audio-cutoff") && more) o->audio_cutoff = atof(argv[++i]);
        else if (!strcmp(argv[i], "--deviation") && more) o->deviation = atof(argv[++i]);
        else if (!strcmp(argv[i], "--spectra") && more) o->spectra = atoi(argv[++i]);
        else if (!strncmp(argv[i], "--spectra-", 10) && more) {
            const char *sub = argv[i] + 10, *value = argv[++i];
            o->spectra_sub = 1;
            if (!strcmp(sub, "hop")) o->spectra_hop = atoi(value);
            else if (!strcmp(sub, "kind")) o->spectra_kind_name = value;
            else if (!strcmp(sub, "window")) o->spectra_window = value;
            else if (!strcmp(sub, "guard")) {
                o->spectra_guard = atoi(value);
                o->spectra_guard_given = 1;
            }
            else if (!strcmp(sub, "fraction")) o->spectra_fraction = atof(value);
            else usage_error(USAGE);
        } else if (!strcmp(argv[i], "--out") && more) o->out_dir = argv[++i];
        else if (argv[i][0] != '-' && o->path == NULL) o->path = argv[i];
        else usage_error(USAGE);
    }
    if (o->det.image_path != NULL) usage_error("--image has no samples to cut out: give a recording");
    if (o->path == NULL) usage_error("no recording file given");
    if (o->size < 1 || o->size > FSEA_EVENTS_MAX_WIDTH) usage_error("--size must be in [1, 1048576]");
    if (o->hop == 0) o->hop = o->size;
    if (o->hop < 1) usage_error("--hop must be positive");
    tool_detector_check(TOOL, &o->det);
    if (o->gap_cols < 0 || o->gap_cols > FSEA_EVENTS_MAX_GAP_COLS) usage_error("--gap-cols must be in [0, 64]");
    if (o->gap_rows < 0 || o->gap_rows > FSEA_EVENTS_MAX_GAP_ROWS) usage_error("--gap-rows must be in [0, 65536]");
    if (o->min_rows < 1 || o->min_rows > 0xffffffffll) usage_error("--min-rows must be at least 1");
    if (o->min_cols < 1 || o->min_cols > 0xffffffffll) usage_error("--min-cols must be at least 1");
    if (o->min_hits < 1) usage_error("--min-hits must be at least 1");
    tool_detector_check_axis(TOOL, &o->det);
    if (o->decimation == 0) usage_error("--decimation D is required");
    if (o->decimation < 1 || o->decimation > FSEA_ZOOM_MAX_DECIMATION) usage_error("--decimation must be in [1, 64]");
    if (o->n_taps < 1 || o->n_taps > FSEA_FIR_MAX_TAPS) usage_error("--taps must be in [1, 512]");
    if (!(o->fill > 0.0 && o->fill <= 1.0)) usage_error("--fill must be in (0, 1]");
    if (o->max_events < 1 || o->max_events > FSEA_EXTRACT_MAX_JOBS) usage_error("--max-events must be in [1, 65536]");
    if (o->max_samples < 1 || o->max_samples > (1ll << 24)) usage_error("--max-samples must be in [1, 16777216]");
    if (o->cutoff < 0.0) usage_error("--cutoff must be positive");
    if (o->lag < 1 || o->lag > FSEA_MEASURE_MAX_LAG) usage_error("--lag must be in [1, 65536]");
    if (o->audio_name != NULL) {
        o->audio_kind = !strcmp(o->audio_name, "fm") ? FSEA_AUDIO_FM : !strcmp(o->audio_name, "am") ? FSEA_AUDIO_AM : -1;
        if (o->audio_kind < 0) usage_error("--audio must be fm or am");
        if (!(o->det.rate > 0.0)) usage_error("--audio needs --rate: the audio rate is in Hz");
        const double ratio = o->det.rate / (double)o->decimation / o->audio_rate;
        if (!(o->audio_rate > 0.0) || !(ratio >= 0.5) || !(ratio < FSEA_AUDIO_MAX_DECIMATION + 0.5)) {
            usage_error("--audio-rate must be RATE / D over a whole number in [1, 64], rounded");
        }
        o->audio_decimation = (int)(ratio + 0.5);
        if (o->audio_taps < 1 || o->audio_taps > FSEA_FIR_MAX_TAPS) usage_error("--audio-taps must be in [1, 512]");
        if (o->audio_cutoff < 0.0) usage_error("--audio-cutoff must be positive");
        if (!(o->deviation > 0.0)) usage_error("--deviation must be positive");
    }
    if (o->spectra != 0) {
        const int n = o->spectra;
        if (n < FSEA_SPECTRA_MIN_N || n > FSEA_SPECTRA_MAX_N || (n & (n - 1)) != 0) usage_error("--spectra must be a power of two in [64, 4096]");
        if (o->spectra_hop == 0) o->spectra_hop = n / 2;
        if (o->spectra_hop < 1 || o->spectra_hop > n) usage_error("--spectra-hop must be in [1, N]");
        const char *kinds[] = {"z", "env", "sq", "fourth"};
        o->spectra_kind = -1;
        for (int k = 0; k < 4; k++) {
            if (!strcmp(o->spectra_kind_name, kinds[k])) o->spectra_kind = k;
        }
        if (o->spectra_kind < 0) usage_error("--spectra-kind must be z, env, sq or fourth");
        o->spectra_window_kind = tool_window_kind(o->spectra_window);
        if (o->spectra_window_kind == TOOL_WINDOW_UNKNOWN) {
            usage_error("--spectra-window must be rect, hann, hamming, blackman, blackmanharris or flattop");
        }
        if (!o->spectra_guard_given) o->spectra_guard = o->spectra_kind == FSEA_SPECTRA_Z ? 0 : 2;
        if (o->spectra_guard < -1 || o->spectra_guard > n / 2 - 1) usage_error("--spectra-guard must be in [-1, N / 2 - 1]");
        if (!(o->spectra_fraction > 0.0 && o->spectra_fraction <= 1.0)) usage_error("--spectra-fraction must be in (0, 1]");
    } else if (o->spectra_sub) {
        usage_error("--spectra-hop, -kind, -window, -guard and -fraction need --spectra N");
    }
    if (o->out_dir == NULL) usage_error("--out DIR is required");
    if (!tool_rows_mode(o->mode_name, "db", &o->mode, &o->type)) usage_error("--mode must be db5, db10 or db");
}

/* A batch whose pairs are resident: its jobs laid out, the event of each, the spans the .cf32 files get -- the outputs
 * without the run-in -- and what every cut-out rests on, the offset of the measures and of the audio. */
typedef struct {
    fsea_extract_job *jobs;
    size_t *event;
    fsea_measure_job *spans;
    size_t n, total; /* jobs; pairs */
    tool_grown pairs;
    double pedestal;
} batch;

/* --measures says what is inside each cut-out.  After a batch's fsea_extract_run_device, with the pairs still resident, one
 * fsea_measure_run_device (include/fsea.h) sums the spans the .cf32 files get -- the outputs without the run-in -- with
 * the lag of --lag (default 1) and the offset (0.5 + 0.5j) sum(c) a cut-out rests on, c the taps as the f32 values the
 * extract object holds.  DIR/measures.txt gets one line per cut-out written:
 *     number pairs power_db freq_cycles freq_mhz width_cycles kurtosis crest dc_re dc_im
 * the eight measures as %.9e (fsea_measure_finish); freq_mhz is what freq_cycles adds to the event's centre_mhz, 0 without
 * --rate.  Without --measures nothing of this happens and no such file is written. */
typedef struct {
    fsea_measure *object;
    fsea_measure_result *results; /* one per job of the run */
    fsea_measure_sums *h_sums;    /* a batch's, on the host and on the device */
    void *d_sums;
} measure_stage;

static void measure_open(measure_stage *m, size_t n_jobs) {
    if (fsea_measure_create(&m->object, 0) != FSEA_OK) die("fsea_measure_create");
    m->results = (fsea_measure_result *)calloc(n_jobs + 1, sizeof(fsea_measure_result));
    m->h_sums = (fsea_measure_sums *)malloc(sizeof(fsea_measure_sums) * (n_jobs + 1));
    if (m->results == NULL || m->h_sums == NULL) usage_error("out of memory");
    if (fsea_device_alloc(0, sizeof(fsea_measure_sums) * (n_jobs + 1), &m->d_sums) != FSEA_OK) die("fsea_device_alloc");
}

static void measure_batch(measure_stage *m, const batch *b, int lag) {
    if (fsea_measure_run_device(m->object, b->pairs.d, b->total, b->spans, b->n, b->pedestal, b->pedestal, lag,
                                (fsea_measure_sums *)m->d_sums, NULL) != FSEA_OK) {
        die("fsea_measure_run_device");
    }
    if (fsea_copy_to_host(0, m->h_sums, m->d_sums, b->n * sizeof(fsea_measure_sums)) != FSEA_OK) die("fsea_copy_to_host");
    for (size_t k = 0; k < b->n; k++) {
        if (fsea_measure_finish(&m->h_sums[k], lag, &m->results[b->event[k]]) != FSEA_OK) die("fsea_measure_finish");
    }
}

static void measure_close(measure_stage *m, const options *o, size_t n_jobs, const size_t *written) {
    FILE *table = open_in(o->out_dir, "%s/measures.txt", 0, "w");
    for (size_t e = 0; e < n_jobs; e++) {
        const fsea_measure_result *r = &m->results[e];
        if (written[e] == 0) continue;
        fprintf(table, "%u %zu %.9e %.9e %.9e %.9e %.9e %.9e %.9e %.9e\n", (unsigned)e, written[e], r->power_db, r->freq_cycles,
                r->freq_cycles * o->det.rate / (double)o->decimation / 1e6, r->width_cycles, r->kurtosis, r->crest, r->dc_re, r->dc_im);
    }
    close_in(table, 0, o->out_dir, "%s/measures.txt", 0);
    fsea_measure_destroy(m->object);
    fsea_device_free(0, m->d_sums);
    free(m->results);
    free(m->h_sums);
}

/* --audio fm|am says what each cut-out carries.  After a batch's fsea_extract_run_device (and the measures), with the pairs
 * still resident, one fsea_audio_run_device (include/fsea.h) demodulates the spans the .cf32 files get: the FM discriminator
 * or the AM envelope, an --audio-taps low-pass (default 41 taps, half amplitude at --audio-cutoff, default 0.4 of the audio
 * rate) and a decimation by D2 = RATE / D over --audio-rate (default 48000), rounded, in [1, 64]; the same offset as the
 * measures.  FM: gain = (RATE / D) / (2 pi --deviation), so a deviation of --deviation Hz (default 75000) is an amplitude of
 * 1; AM: gain 1 and the cut-out's mean taken off on the host.  DIR/cutout-%05u.wav is mono 16-bit PCM at RATE / D / D2 (the
 * header's rate rounded to a whole number), sample = (int16_t)(audio * 32000) as nrf_player's, saturated; DIR/audio.txt gets
 * one line per file:
 *     number rate samples peak
 * (peak: the largest |audio| written, before the scale), and the summary line gains ` audio A`, the files written.  Without
 * --audio nothing of this happens. */
typedef struct {
    fsea_audio *object;
    fsea_audio_job *jobs; /* a batch's */
    tool_grown audio;     /* and their audio, on the device and on the host */
    size_t n_files;
    double out_rate, gain;
    FILE *list;           /* DIR/audio.txt: main opens it once DIR is there */
} audio_stage;

static void audio_open(audio_stage *a, const options *o, size_t n_jobs) {
    const double pair_rate = o->det.rate / (double)o->decimation;
    a->out_rate = pair_rate / (double)o->audio_decimation;
    a->gain = o->audio_kind == FSEA_AUDIO_FM ? pair_rate / (2.0 * 3.14159265358979323846 * o->deviation) : 1.0;
    double *c = (double *)malloc(sizeof(double) * (size_t)o->audio_taps);
    a->jobs = (fsea_audio_job *)malloc(sizeof(fsea_audio_job) * (n_jobs + 1));
    if (c == NULL || a->jobs == NULL) usage_error("out of memory");
    const double cutoff = o->audio_cutoff == 0.0 ? 0.4 * a->out_rate : o->audio_cutoff;
    if (fsea_fir_lowpass_taps(pair_rate, cutoff, o->audio_taps, c) != FSEA_OK) die("fsea_fir_lowpass_taps");
    if (fsea_audio_create(&a->object, o->audio_kind, c, o->audio_taps, o->audio_decimation, 0) != FSEA_OK) die("fsea_audio_create");
    free(c);
}

/* every span's audio back to back, demodulated and brought to the host; then the .wav and the line of every cut-out that has some */
static void audio_batch(audio_stage *a, const batch *b, const options *o) {
    size_t total = 0;
    for (size_t k = 0; k < b->n; k++) a->jobs[k] = (fsea_audio_job){b->spans[k].first_pair, b->spans[k].n_pairs, 0};
    if (fsea_audio_layout(a->object, a->jobs, b->n, &total) != FSEA_OK) die("fsea_audio_layout");
    if (total == 0) return;
    tool_grown_need(TOOL, &a->audio, total, sizeof(float), 1);
    if (fsea_audio_run_device(a->object, b->pairs.d, b->total, a->jobs, b->n, b->pedestal, b->pedestal, a->gain, (float *)a->audio.d, total,
                              NULL) != FSEA_OK) {
        die("fsea_audio_run_device");
    }
    if (fsea_copy_to_host(0, a->audio.h, a->audio.d, total * sizeof(float)) != FSEA_OK) die("fsea_copy_to_host");
    for (size_t k = 0; k < b->n; k++) {
        const size_t n_audio = (size_t)a->jobs[k].n_pairs / (size_t)o->audio_decimation;
        const float *x = (const float *)a->audio.h + a->jobs[k].out_first;
        const unsigned e = (unsigned)b->event[k];
        double mean = 0.0, peak;
        if (n_audio == 0) continue;
        if (o->audio_kind == FSEA_AUDIO_AM) { /* the carrier's level: the sum in order, over the count */
            for (size_t i = 0; i < n_audio; i++) mean += (double)x[i];
            mean /= (double)n_audio;
        }
        FILE *wav = open_in(o->out_dir, "%s/cutout-%05u.wav", e, "wb");
        close_in(wav, write_wav(wav, (uint32_t)(a->out_rate + 0.5), x, mean, n_audio, &peak), o->out_dir, "%s/cutout-%05u.wav", e);
        fprintf(a->list, "%u %.3f %zu %.6f\n", e, a->out_rate, n_audio, peak);
        a->n_files++;
    }
}

static void audio_close(audio_stage *a, const options *o) {
    close_in(a->list, 0, o->out_dir, "%s/audio.txt", 0);
    fsea_audio_destroy(a->object);
    tool_grown_free(&a->audio);
    free(a->jobs);
}

/* --spectra N says what each cut-out looks like in frequency.  After a batch's fsea_extract_run_device (and the other stages),
 * with the pairs still resident, one fsea_spectra_run_device (include/fsea.h) averages the periodograms of the spans the
 * .cf32 files get: N bins every --spectra-hop pairs (default N / 2) under --spectra-window (default hann), of the kind
 * --spectra-kind (default z); the same offset as the measures.  fsea_spectra_finish makes the figures of each row with
 * --spectra-guard (default 0 for z, 2 otherwise) and --spectra-fraction (default 0.99).  DIR/spectra.txt gets one line per
 * cut-out written:
 *     number segments obw centroid line line_db
 * obw, centroid and line as %.9e in Hz with --rate (obw_bins / N, centroid_cycles and peak_cycles times RATE / D), in
 * cycles per pair without; a cut-out shorter than N pairs gets `number 0 short: P pairs, fewer than N`.  The summary line
 * gains ` spectra P`, the cut-outs that have a spectrum.  Without --spectra nothing of this happens. */
typedef struct {
    fsea_spectra *object;
    fsea_spectra_job *jobs; /* a batch's */
    tool_grown power;       /* and their rows, on the device and on the host */
    size_t n_rows;
    FILE *list;             /* DIR/spectra.txt: main opens it once DIR is there */
} spectra_stage;

static void spectra_open(spectra_stage *s, const options *o, size_t n_jobs) {
    float *w = (float *)malloc(sizeof(float) * (size_t)o->spectra);
    s->jobs = (fsea_spectra_job *)malloc(sizeof(fsea_spectra_job) * (n_jobs + 1));
    if (w == NULL || s->jobs == NULL) usage_error("out of memory");
    if (fsea_window_fill(o->spectra_window_kind, o->spectra, w) != FSEA_OK) die("fsea_window_fill");
    if (fsea_spectra_create(&s->object, o->spectra, o->spectra_hop, o->spectra_kind, o->spectra_window_kind == FSEA_WINDOW_RECT ? NULL : w,
                            0) != FSEA_OK) {
        die("fsea_spectra_create");
    }
    free(w);
}

/* every span's row back to back, averaged and brought to the host; then the line of every cut-out written */
static void spectra_batch(spectra_stage *s, const batch *b, const options *o) {
    size_t total = 0;
    const double unit = o->det.rate > 0.0 ? o->det.rate / (double)o->decimation : 1.0;
    for (size_t k = 0; k < b->n; k++) s->jobs[k] = (fsea_spectra_job){b->spans[k].first_pair, b->spans[k].n_pairs, 0};
    if (fsea_spectra_layout(s->object, s->jobs, b->n, &total) != FSEA_OK) die("fsea_spectra_layout");
    if (total != 0) {
        tool_grown_need(TOOL, &s->power, total, sizeof(float), 1);
        if (fsea_spectra_run_device(s->object, b->pairs.d, b->total, s->jobs, b->n, b->pedestal, b->pedestal, (float *)s->power.d, total,
                                    NULL) != FSEA_OK) {
            die("fsea_spectra_run_device");
        }
        if (fsea_copy_to_host(0, s->power.h, s->power.d, total * sizeof(float)) != FSEA_OK) die("fsea_copy_to_host");
    }
    for (size_t k = 0; k < b->n; k++) {
        const size_t n_pairs = (size_t)s->jobs[k].n_pairs, segments = fsea_spectra_segments(s->object, n_pairs);
        const unsigned e = (unsigned)b->event[k];
        fsea_spectra_result r;
        if (n_pairs == 0) continue; /* no cut-out is written */
        if (segments == 0) {
            fprintf(s->list, "%u 0 short: %zu pairs, fewer than %d\n", e, n_pairs, o->spectra);
            continue;
        }
        if (fsea_spectra_finish((const float *)s->power.h + s->jobs[k].out_first, o->spectra, o->spectra_guard, o->spectra_fraction, &r) != FSEA_OK) {
            die("fsea_spectra_finish");
        }
        fprintf(s->list, "%u %zu %.9e %.9e %.9e %.9e\n", e, segments, (double)r.obw_bins / (double)o->spectra * unit, r.centroid_cycles * unit,
                r.peak_cycles * unit, r.line_db);
        s->n_rows++;
    }
}

static void spectra_close(spectra_stage *s, const options *o) {
    close_in(s->list, 0, o->out_dir, "%s/spectra.txt", 0);
    fsea_spectra_destroy(s->object);
    tool_grown_free(&s->power);
    free(s->jobs);
}

int main(int argc, char **argv) {
    options o = {.window = "rect", .mode_name = "db5", .n_taps = 97, .lag = 1, .audio_taps = 41, .min_rows = 1, .min_cols = 1,
                 .min_hits = 1, .max_events = 1024, .max_samples = 1ll << 24, .fill = 0.8, .audio_rate = 48000.0, .deviation = 75000.0,
                 .det = TOOL_DETECTOR_DEFAULTS, .audio_kind = -1, .audio_decimation = 1, .spectra_kind_name = "z", .spectra_window = "hann",
                 .spectra_fraction = 0.99};
    parse_options(argc, argv, &o);
    const int size = o.size, hop = o.hop, decimation = o.decimation, n_taps = o.n_taps;
    const double rate = o.det.rate, freq = o.det.freq;

    /* pass 1: fsea-events' */
    tool_row_source src;
    tool_detector_check_chunk(TOOL, &o.det, size, hop, o.type);
    tool_rows_open(&src, TOOL, o.path, size, hop, o.mode, o.window, o.flip);
    tool_rows_keep(&src, tool_detector_keep(&o.det, size, o.type));
    tool_detector_object detector = tool_detector_create(TOOL, &o.det, size);
    fsea_events *events = NULL;
    if (fsea_events_create(&events, size, 0) != FSEA_OK) die("fsea_events_create");
    if (fsea_events_set_gap(events, o.gap_cols) != FSEA_OK) die("fsea_events_set_gap");
    tool_run_list runs = {NULL, 0, 0};
    const size_t done = tool_recording_runs(TOOL, &src, &detector, events, o.type, &runs);
    tool_rows_close(&src);
    if (done < 1) return tool_rows_none(TOOL, o.path, size);
    size_t n_events = 0;
    fsea_events_event *found_events = tool_link(TOOL, &runs, o.gap_cols, o.gap_rows, o.min_rows, o.min_cols, o.min_hits, NULL, &n_events);

    /* pass 2: the first max_events events as jobs */
    FILE *fp = fopen(o.path, "rb");
    if (fp == NULL || fseek(fp, 0, SEEK_END) != 0) usage_error("cannot read the recording again");
    const uint64_t n_samples = (uint64_t)ftell(fp) / 2;
    const size_t n_jobs = n_events < (size_t)o.max_events ? n_events : (size_t)o.max_events;
    const size_t lead_out = fsea_extract_lead(n_taps, decimation) / (size_t)decimation;
    fsea_extract_job *jobs = (fsea_extract_job *)malloc(sizeof(fsea_extract_job) * (n_jobs + 1));
    uint8_t *fits = (uint8_t *)calloc(n_jobs + 1, 1), *cut = (uint8_t *)calloc(n_jobs + 1, 1);
    size_t *written = (size_t *)calloc(n_events + 1, sizeof(size_t));
    double *taps = (double *)malloc(sizeof(double) * (size_t)n_taps);
    if (jobs == NULL || fits == NULL || cut == NULL || written == NULL || taps == NULL) usage_error("out of memory");
    if (fsea_extract_jobs(found_events, n_jobs, size, hop, n_samples, n_taps, decimation, o.fill, jobs, fits) != FSEA_OK) die("fsea_extract_jobs");
    for (size_t j = 0; j < n_jobs; j++) {
        if (jobs[j].n_samples > (uint64_t)o.max_samples) {
            jobs[j].n_samples = (uint64_t)o.max_samples;
            cut[j] = 1;
        }
    }
    /* the design takes a rate and a frequency in the same unit: without --rate, 1 and cycles per sample */
    const double design_rate = rate > 0.0 ? rate : 1.0;
    const double cutoff = o.cutoff == 0.0 ? 0.4 * design_rate / (double)decimation : o.cutoff;
    if (fsea_fir_lowpass_taps(design_rate, cutoff, n_taps, taps) != FSEA_OK) die("fsea_fir_lowpass_taps");
    fsea_extract *extract = NULL;
    if (fsea_extract_create(&extract, taps, n_taps, decimation, 0) != FSEA_OK) die("fsea_extract_create");
    /* what can fail before anything is written: the stages' objects, audio's first, then DIR and audio's list in it */
    measure_stage measure = {0};
    audio_stage audio = {0};
    spectra_stage spectra = {0};
    if (o.audio_kind >= 0) audio_open(&audio, &o, n_jobs);
    if (o.spectra) spectra_open(&spectra, &o, n_jobs);
    if (o.measures) measure_open(&measure, n_jobs);
    if (mkdir(o.out_dir, 0777) != 0 && errno != EEXIST) {
        fprintf(stderr, TOOL ": cannot create directory %s\n", o.out_dir);
        return EXIT_FAILURE;
    }
    batch b = {(fsea_extract_job *)malloc(sizeof(fsea_extract_job) * (n_jobs + 1)), (size_t *)malloc(sizeof(size_t) * (n_jobs + 1)),
               (fsea_measure_job *)malloc(sizeof(fsea_measure_job) * (n_jobs + 1)), 0, 0, {NULL, NULL, 0}, 0.0};
    out_name_len = strlen(o.out_dir) + 32;
    out_name = (char *)malloc(out_name_len);
    if (out_name == NULL || b.jobs == NULL || b.event == NULL || b.spans == NULL) usage_error("out of memory");
    if (o.audio_kind >= 0) audio.list = open_in(o.out_dir, "%s/audio.txt", 0, "w");
    if (o.spectra) spectra.list = open_in(o.out_dir, "%s/spectra.txt", 0, "w");
    for (int k = 0; k < n_taps; k++) b.pedestal += (double)(float)taps[k];
    b.pedestal *= 0.5; /* of the taps as the f32 values the extract holds */
    void *h_iq = NULL, *d_iq = NULL;
    size_t n_cutouts = 0;
    if (fsea_host_alloc(2 * BATCH_SAMPLES, &h_iq) != FSEA_OK) die("fsea_host_alloc");
    if (fsea_device_alloc(0, 2 * BATCH_SAMPLES, &d_iq) != FSEA_OK) die("fsea_device_alloc");
    for (size_t j = 0; j < n_jobs;) {
        /* read the batch: the jobs from j on whose samples fit the buffer, back to back */
        size_t at = 0;
        for (b.n = 0; j < n_jobs && at + (size_t)jobs[j].n_samples <= BATCH_SAMPLES; j++) {
            if (jobs[j].n_samples == 0) continue;
            if (fseek(fp, (long)(2 * jobs[j].first), SEEK_SET) != 0 ||
                fread((uint8_t *)h_iq + 2 * at, 2, (size_t)jobs[j].n_samples, fp) != (size_t)jobs[j].n_samples) {
                fprintf(stderr, TOOL ": short read of %s\n", o.path);
                return EXIT_FAILURE;
            }
            b.jobs[b.n] = jobs[j];
            b.jobs[b.n].first = at;   /* its place in the buffer; sample_offset stays the stream position */
            b.event[b.n++] = j;
            at += (size_t)jobs[j].n_samples;
        }
        if (b.n == 0) continue;
        /* lay it out, upload, extract; then the stages on the resident pairs, the pairs to the host, the files */
        if (fsea_extract_layout(extract, b.jobs, b.n, &b.total) != FSEA_OK) die("fsea_extract_layout");
        if (b.total == 0) continue;
        /* with or without the stages: a job has at most 2^24 samples (--max-samples), fsea_measure_jobs' own cap of a span */
        if (fsea_measure_jobs(b.jobs, b.n, decimation, lead_out, b.spans) != FSEA_OK) die("fsea_measure_jobs");
        tool_grown_need(TOOL, &b.pairs, b.total, 2 * sizeof(float), 1);
        if (fsea_copy_to_device(0, d_iq, h_iq, 2 * at) != FSEA_OK) die("fsea_copy_to_device");
        if (fsea_extract_run_device(extract, d_iq, at, o.flip, b.jobs, b.n, b.pairs.d, b.total, NULL) != FSEA_OK) die("fsea_extract_run_device");
        if (o.measures) measure_batch(&measure, &b, o.lag);
        if (o.audio_kind >= 0) audio_batch(&audio, &b, &o);
        if (o.spectra) spectra_batch(&spectra, &b, &o);
        if (fsea_copy_to_host(0, b.pairs.h, b.pairs.d, b.total * 2 * sizeof(float)) != FSEA_OK) die("fsea_copy_to_host");
        for (size_t k = 0; k < b.n; k++) {
            const size_t keep = (size_t)b.spans[k].n_pairs, e = b.event[k];
            if (keep == 0) continue;
            const float *from = (const float *)b.pairs.h + 2 * (size_t)b.spans[k].first_pair;
            FILE *out = open_in(o.out_dir, "%s/cutout-%05u.cf32", (unsigned)e, "wb");
            close_in(out, fwrite(from, 2 * sizeof(float), keep, out) != keep, o.out_dir, "%s/cutout-%05u.cf32", (unsigned)e);
            written[e] = keep;
            n_cutouts++;
        }
    }

    FILE *list = open_in(o.out_dir, "%s/cutouts.txt", 0, "w");
    for (size_t e = 0; e < n_events; e++) {
        const fsea_events_event *ev = &found_events[e];
        const int listed = e < n_jobs;
        const double mhz = rate > 0.0 ? 0.5 * (tool_column_mhz(freq, rate, size, ev->col_first) + tool_column_mhz(freq, rate, size, ev->col_last)) : 0.0;
        fprintf(list, "%u %u %u %u %u %llu %llu %.6f %.3f %zu %d %d\n", (unsigned)e, ev->row_first, ev->row_last, ev->col_first,
                ev->col_last, listed ? (unsigned long long)jobs[e].first : 0ull, listed ? (unsigned long long)jobs[e].n_samples : 0ull, mhz,
                rate / (double)decimation, written[e], listed ? (int)fits[e] : 0, listed ? (int)cut[e] : 0);
    }
    close_in(list, 0, o.out_dir, "%s/cutouts.txt", 0);
    if (o.measures) measure_close(&measure, &o, n_jobs, written);
    if (o.audio_kind >= 0) audio_close(&audio, &o);
    if (o.spectra) spectra_close(&spectra, &o);
    printf("rows %zu runs %zu events %zu cutouts %zu skipped %zu", done, runs.n, n_events, n_cutouts, n_events - n_cutouts);
    if (o.audio_kind >= 0) printf(" audio %zu", audio.n_files);
    if (o.spectra) printf(" spectra %zu", spectra.n_rows);
    putchar('\n');

    fsea_extract_destroy(extract);
    fsea_events_destroy(events);
    tool_detector_destroy(&detector);
    fsea_device_free(0, d_iq);
    tool_grown_free(&b.pairs);
    fsea_host_free(h_iq);
    fclose(fp);
    free(out_name);
    free(b.jobs);
    free(b.event);
    free(b.spans);
    free(jobs);
    free(fits);
    free(cut);
    free(written);
    free(taps);
    free(found_events);
    free(runs.runs);
    return 0;
}
