/*
 * fsea-cutouts -- from a recording to one IQ file per emission: fsea-events finds the time-frequency boxes, this tool turns
 * each box back into its signal, mixed to the centre, low-passed and decimated by D.
 *
 * Pass 1 is fsea-events' for a recording: every frame of N samples (one every H) through a plan in a dB mode, the rows to a
 * fsea_cfar object with a mask, mask and rows to a fsea_events object, all on the device chunk by chunk; the runs are kept
 * on the host and linked once at the end (tool_common.h).  Pass 2 turns the first --max-events surviving events into jobs with
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
 * --measures says what is inside each cut-out.  After a batch's fsea_extract_run_device, with the pairs still resident, one
 * fsea_measure_run_device (include/fsea.h) sums the spans the .cf32 files get -- the outputs without the run-in -- with
 * the lag of --lag (default 1) and the offset (0.5 + 0.5j) sum(c) a cut-out rests on, c the taps as the f32 values the
 * extract object holds.  DIR/measures.txt gets one line per cut-out written:
 *     number pairs power_db freq_cycles freq_mhz width_cycles kurtosis crest dc_re dc_im
 * the eight measures as %.9e (fsea_measure_finish); freq_mhz is what freq_cycles adds to the event's centre_mhz, 0 without
 * --rate.  Without --measures nothing of this happens and no such file is written.
 *
 * --audio fm|am says what each cut-out carries.  After a batch's fsea_extract_run_device (and the measures), with the pairs
 * still resident, one fsea_audio_run_device (include/fsea.h) demodulates the spans the .cf32 files get: the FM discriminator
 * or the AM envelope, an --audio-taps low-pass (default 41 taps, half amplitude at --audio-cutoff, default 0.4 of the audio
 * rate) and a decimation by D2 = RATE / D over --audio-rate (default 48000), rounded, in [1, 64]; the same offset as the
 * measures.  FM: gain = (RATE / D) / (2 pi --deviation), so a deviation of --deviation Hz (default 75000) is an amplitude of
 * 1; AM: gain 1 and the cut-out's mean taken off on the host.  DIR/cutout-%05u.wav is mono 16-bit PCM at RATE / D / D2 (the
 * header's rate rounded to a whole number), sample = (int16_t)(audio * 32000) as nrf_player's, saturated; DIR/audio.txt gets
 * one line per file:
 *     number rate samples peak
 * (peak: the largest |audio| written, before the scale), and the summary line gains ` audio A`, the files written.  Without
 * --audio nothing of this happens.
 *
 * usage: fsea-cutouts FILE --size N --decimation D --out DIR [--hop H] [--window NAME] [--flip] [--mode db5|db10|db]
 *                     [--guard G] [--train T] [--offset LEVELS] [--method ca|go|so] [--gap-cols B] [--gap-rows R]
 *                     [--min-rows R] [--min-cols B] [--min-hits K] [--rate HZ --freq MHZ] [--taps L] [--cutoff HZ]
 *                     [--fill F] [--max-events E] [--max-samples S] [--measures [--lag K]]
 *                     [--audio fm|am [--audio-rate HZ] [--audio-taps N] [--audio-cutoff HZ] [--deviation HZ]]
 */
#include <errno.h>
#include <limits.h>
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
    "                    [--guard G] [--train T] [--offset LEVELS] [--method ca|go|so] [--gap-cols B] [--gap-rows R]\n"
    "                    [--min-rows R] [--min-cols B] [--min-hits K] [--rate HZ --freq MHZ] [--taps L] [--cutoff HZ]\n"
    "                    [--fill F] [--max-events E] [--max-samples S] [--measures [--lag K]]\n"
    "                    [--audio fm|am [--audio-rate HZ] [--audio-taps N] [--audio-cutoff HZ] [--deviation HZ]]\n"
    "  FILE is a raw 8-bit IQ recording (--flip: HackRF int8).  The emissions are found as fsea-events finds them (its\n"
    "  options, same defaults); each one whose columns times D fill at most F of the N columns is mixed to the centre,\n"
    "  low-passed (L taps, half amplitude at --cutoff, default 0.4 RATE / D) and decimated by D on the GPU, all of a batch in\n"
    "  one launch, and written to DIR/cutout-NNNNN.cf32 as f32 pairs; DIR/cutouts.txt lists every event.  A cut-out longer\n"
    "  than S samples is cut short.  --measures: DIR/measures.txt says of every cut-out written its power in dB, its\n"
    "  frequency offset (lag K pairs, default 1), spectrum width, envelope kurtosis, crest factor and what is left of its DC.\n"
    "  --audio: every cut-out written is FM- or AM-demodulated on the GPU, low-passed (N taps, half amplitude at\n"
    "  --audio-cutoff, default 0.4 of the audio rate) and decimated to about --audio-rate; DIR/cutout-NNNNN.wav is mono 16-bit\n"
    "  PCM, full scale at --deviation for FM, and DIR/audio.txt lists number, rate, samples and peak of every file.  Needs --rate.\n"
    "  Prints `rows R runs N events E cutouts C skipped S`, with --audio followed by ` audio A`\n"
    "  defaults: --taps 97 --fill 0.8 --max-events 1024 --max-samples 16777216 --audio-rate 48000 --audio-taps 41 --deviation 75000";

static void usage_error(const char *msg) { tool_usage_error(TOOL, msg); }

static void die(const char *what) { tool_die(TOOL, what); }

/* 16 and 32 bits, little-endian */
static void put_le(uint8_t *at, uint32_t value, int bytes) {
    for (int i = 0; i < bytes; i++) at[i] = (uint8_t)(value >> (8 * i));
}

/* DIR/cutout-NNNNN.wav: the 44-byte header of mono 16-bit PCM and n samples; 0 when everything was written */
static int write_wav(const char *name, uint32_t rate, const int16_t *pcm, size_t n) {
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
    FILE *out = fopen(name, "wb");
    if (out == NULL) return 1;
    int bad = fwrite(head, 1, sizeof(head), out) != sizeof(head);
    for (size_t i = 0; i < n && !bad; i++) {
        uint8_t two[2];
        put_le(two, (uint16_t)pcm[i], 2);
        bad = fwrite(two, 1, 2, out) != 2;
    }
    return (fclose(out) != 0) | bad;
}

/* a file of the output that could not be written, for main's exit status */
static int cannot_write(const char *name) {
    fprintf(stderr, TOOL ": cannot write %s\n", name);
    return EXIT_FAILURE;
}

int main(int argc, char **argv) {
    const char *path = NULL, *out_dir = NULL, *window = "rect", *mode_name = "db5";
    int size = 0, hop = 0, flip = 0, gap_cols = 0, gap_rows = 0, decimation = 0, n_taps = 97, measures = 0, lag = 1;
    long long min_rows = 1, min_cols = 1, min_hits = 1, max_events = 1024, max_samples = 1ll << 24;
    double cutoff = 0.0, fill = 0.8, audio_rate = 48000.0, audio_cutoff = 0.0, deviation = 75000.0;
    const char *audio_name = NULL;
    int audio_taps = 41;
    tool_detector det = TOOL_DETECTOR_DEFAULTS;
    for (int i = 1; i < argc; i++) {
        const int more = i + 1 < argc;
        if (!strcmp(argv[i], "--help")) {
            puts(USAGE);
            return 0;
        } else if (!strcmp(argv[i], "--size") && more) size = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--hop") && more) hop = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--window") && more) window = argv[++i];
        else if (!strcmp(argv[i], "--flip")) flip = 1;
        else if (!strcmp(argv[i], "--mode") && more) mode_name = argv[++i];
        else if (tool_detector_option(TOOL, &det, argc, argv, &i)) continue;
        else if (!strcmp(argv[i], "--gap-cols") && more) gap_cols = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gap-rows") && more) gap_rows = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--min-rows") && more) min_rows = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-cols") && more) min_cols = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--min-hits") && more) min_hits = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--decimation") && more) decimation = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--taps") && more) n_taps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--cutoff") && more) cutoff = atof(argv[++i]);
        else if (!strcmp(argv[i], "--fill") && more) fill = atof(argv[++i]);
        else if (!strcmp(argv[i], "--max-events") && more) max_events = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--max-samples") && more) max_samples = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--measures")) measures = 1;
        else if (!strcmp(argv[i], "--lag") && more) lag = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--audio") && more) audio_name = argv[++i];
        else if (!strcmp(argv[i], "--audio-rate") && more) audio_rate = atof(argv[++i]);
        else if (!strcmp(argv[i], "--audio-taps") && more) audio_taps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--audio-cutoff") && more) audio_cutoff = atof(argv[++i]);
        else if (!strcmp(argv[i], "--deviation") && more) deviation = atof(argv[++i]);
        else if (!strcmp(argv[i], "--out") && more) out_dir = argv[++i];
        else if (argv[i][0] != '-' && path == NULL) path = argv[i];
        else usage_error(USAGE);
    }
    const double rate = det.rate, freq = det.freq;
    if (det.image_path != NULL) usage_error("--image has no samples to cut out: give a recording");
    if (path == NULL) usage_error("no recording file given");
    if (size < 1 || size > FSEA_EVENTS_MAX_WIDTH) usage_error("--size must be in [1, 1048576]");
    if (hop == 0) hop = size;
    if (hop < 1) usage_error("--hop must be positive");
    tool_detector_check(TOOL, &det);
    if (gap_cols < 0 || gap_cols > FSEA_EVENTS_MAX_GAP_COLS) usage_error("--gap-cols must be in [0, 64]");
    if (gap_rows < 0 || gap_rows > FSEA_EVENTS_MAX_GAP_ROWS) usage_error("--gap-rows must be in [0, 65536]");
    if (min_rows < 1 || min_rows > 0xffffffffll) usage_error("--min-rows must be at least 1");
    if (min_cols < 1 || min_cols > 0xffffffffll) usage_error("--min-cols must be at least 1");
    if (min_hits < 1) usage_error("--min-hits must be at least 1");
    tool_detector_check_axis(TOOL, &det);
    if (decimation == 0) usage_error("--decimation D is required");
    if (decimation < 1 || decimation > FSEA_ZOOM_MAX_DECIMATION) usage_error("--decimation must be in [1, 64]");
    if (n_taps < 1 || n_taps > FSEA_FIR_MAX_TAPS) usage_error("--taps must be in [1, 512]");
    if (!(fill > 0.0 && fill <= 1.0)) usage_error("--fill must be in (0, 1]");
    if (max_events < 1 || max_events > FSEA_EXTRACT_MAX_JOBS) usage_error("--max-events must be in [1, 65536]");
    if (max_samples < 1 || max_samples > (1ll << 24)) usage_error("--max-samples must be in [1, 16777216]");
    if (cutoff < 0.0) usage_error("--cutoff must be positive");
    if (lag < 1 || lag > FSEA_MEASURE_MAX_LAG) usage_error("--lag must be in [1, 65536]");
    int audio_kind = -1, audio_decimation = 1;
    if (audio_name != NULL) {
        audio_kind = !strcmp(audio_name, "fm") ? FSEA_AUDIO_FM : !strcmp(audio_name, "am") ? FSEA_AUDIO_AM : -1;
        if (audio_kind < 0) usage_error("--audio must be fm or am");
        if (!(rate > 0.0)) usage_error("--audio needs --rate: the audio rate is in Hz");
        if (decimation >= 1 && decimation <= FSEA_ZOOM_MAX_DECIMATION) {
            const double ratio = rate / (double)decimation / audio_rate;
            if (!(audio_rate > 0.0) || !(ratio >= 0.5) || !(ratio < FSEA_AUDIO_MAX_DECIMATION + 0.5)) {
                usage_error("--audio-rate must be RATE / D over a whole number in [1, 64], rounded");
            }
            audio_decimation = (int)(ratio + 0.5);
        }
        if (audio_taps < 1 || audio_taps > FSEA_FIR_MAX_TAPS) usage_error("--audio-taps must be in [1, 512]");
        if (audio_cutoff < 0.0) usage_error("--audio-cutoff must be positive");
        if (!(deviation > 0.0)) usage_error("--deviation must be positive");
    }
    if (out_dir == NULL) usage_error("--out DIR is required");
    int mode = 0, type = 0;
    if (!tool_rows_mode(mode_name, "db", &mode, &type)) usage_error("--mode must be db5, db10 or db");

    /* pass 1: fsea-events' */
    tool_row_source src;
    tool_rows_open(&src, TOOL, path, size, hop, mode, window, flip);
    fsea_cfar *cfar = tool_detector_create(TOOL, &det, size);
    fsea_events *events = NULL;
    if (fsea_events_create(&events, size, 0) != FSEA_OK) die("fsea_events_create");
    if (fsea_events_set_gap(events, gap_cols) != FSEA_OK) die("fsea_events_set_gap");
    tool_run_list runs = {NULL, 0, 0};
    const size_t done = tool_recording_runs(TOOL, &src, cfar, events, type, &runs);
    tool_rows_close(&src);
    if (done < 1) return tool_rows_none(TOOL, path, size);
    size_t n_events = 0;
    fsea_events_event *found_events = tool_link(TOOL, &runs, gap_cols, gap_rows, min_rows, min_cols, min_hits, NULL, &n_events);

    /* pass 2: the first max_events events as jobs */
    FILE *fp = fopen(path, "rb");
    if (fp == NULL || fseek(fp, 0, SEEK_END) != 0) usage_error("cannot read the recording again");
    const uint64_t n_samples = (uint64_t)ftell(fp) / 2;
    const size_t n_jobs = n_events < (size_t)max_events ? n_events : (size_t)max_events;
    const size_t lead_out = fsea_extract_lead(n_taps, decimation) / (size_t)decimation;
    fsea_extract_job *jobs = (fsea_extract_job *)malloc(sizeof(fsea_extract_job) * (n_jobs + 1));
    uint8_t *fits = (uint8_t *)calloc(n_jobs + 1, 1), *cut = (uint8_t *)calloc(n_jobs + 1, 1);
    size_t *written = (size_t *)calloc(n_events + 1, sizeof(size_t));
    double *taps = (double *)malloc(sizeof(double) * (size_t)n_taps);
    if (jobs == NULL || fits == NULL || cut == NULL || written == NULL || taps == NULL) usage_error("out of memory");
    if (fsea_extract_jobs(found_events, n_jobs, size, hop, n_samples, n_taps, decimation, fill, jobs, fits) != FSEA_OK) die("fsea_extract_jobs");
    for (size_t j = 0; j < n_jobs; j++) {
        if (jobs[j].n_samples > (uint64_t)max_samples) {
            jobs[j].n_samples = (uint64_t)max_samples;
            cut[j] = 1;
        }
    }
    /* the design takes a rate and a frequency in the same unit: without --rate, 1 and cycles per sample */
    const double design_rate = rate > 0.0 ? rate : 1.0;
    if (cutoff == 0.0) cutoff = 0.4 * design_rate / (double)decimation;
    if (fsea_fir_lowpass_taps(design_rate, cutoff, n_taps, taps) != FSEA_OK) die("fsea_fir_lowpass_taps");
    fsea_extract *extract = NULL;
    if (fsea_extract_create(&extract, taps, n_taps, decimation, 0) != FSEA_OK) die("fsea_extract_create");
    /* --measures: the object, one record per event, and the pedestal of a cut-out from the taps as the extract holds them */
    fsea_measure *measure = NULL;
    fsea_measure_result *measured = NULL;
    fsea_measure_job *spans = NULL;
    fsea_measure_sums *h_sums = NULL;
    void *d_sums = NULL;
    double pedestal = 0.0;
    if (measures || audio_kind >= 0) {
        for (int k = 0; k < n_taps; k++) pedestal += (double)(float)taps[k];
        pedestal *= 0.5;
    }
    /* --audio: the object, the spans and their audio jobs, the audio of a batch on the device and on the host */
    fsea_audio *audio = NULL;
    fsea_measure_job *audio_spans = NULL;
    fsea_audio_job *audio_jobs = NULL;
    void *d_audio = NULL;
    float *h_audio = NULL;
    int16_t *pcm = NULL;
    size_t audio_cap = 0, pcm_cap = 0, n_audio_files = 0;
    double out_rate = 0.0, audio_gain = 1.0;
    FILE *audio_list = NULL;
    if (audio_kind >= 0) {
        const double pair_rate = rate / (double)decimation;
        out_rate = pair_rate / (double)audio_decimation;
        if (audio_cutoff == 0.0) audio_cutoff = 0.4 * out_rate;
        double *audio_c = (double *)malloc(sizeof(double) * (size_t)audio_taps);
        audio_spans = (fsea_measure_job *)malloc(sizeof(fsea_measure_job) * (n_jobs + 1));
        audio_jobs = (fsea_audio_job *)malloc(sizeof(fsea_audio_job) * (n_jobs + 1));
        if (audio_c == NULL || audio_spans == NULL || audio_jobs == NULL) usage_error("out of memory");
        if (fsea_fir_lowpass_taps(pair_rate, audio_cutoff, audio_taps, audio_c) != FSEA_OK) die("fsea_fir_lowpass_taps");
        if (fsea_audio_create(&audio, audio_kind, audio_c, audio_taps, audio_decimation, 0) != FSEA_OK) die("fsea_audio_create");
        free(audio_c);
        if (audio_kind == FSEA_AUDIO_FM) audio_gain = pair_rate / (2.0 * 3.14159265358979323846 * deviation);
    }
    if (measures) {
        if (fsea_measure_create(&measure, 0) != FSEA_OK) die("fsea_measure_create");
        measured = (fsea_measure_result *)calloc(n_jobs + 1, sizeof(fsea_measure_result));
        spans = (fsea_measure_job *)malloc(sizeof(fsea_measure_job) * (n_jobs + 1));
        h_sums = (fsea_measure_sums *)malloc(sizeof(fsea_measure_sums) * (n_jobs + 1));
        if (measured == NULL || spans == NULL || h_sums == NULL) usage_error("out of memory");
        if (fsea_device_alloc(0, sizeof(fsea_measure_sums) * (n_jobs + 1), &d_sums) != FSEA_OK) die("fsea_device_alloc");
    }
    if (mkdir(out_dir, 0777) != 0 && errno != EEXIST) {
        fprintf(stderr, TOOL ": cannot create directory %s\n", out_dir);
        return EXIT_FAILURE;
    }

    size_t name_len = strlen(out_dir) + 32, n_cutouts = 0;
    char *name = (char *)malloc(name_len);
    if (audio_kind >= 0 && name != NULL) {
        snprintf(name, name_len, "%s/audio.txt", out_dir);
        audio_list = fopen(name, "w");
        if (audio_list == NULL) return cannot_write(name);
    }
    fsea_extract_job *batch = (fsea_extract_job *)malloc(sizeof(fsea_extract_job) * (n_jobs + 1));
    size_t *batch_of = (size_t *)malloc(sizeof(size_t) * (n_jobs + 1));
    void *h_iq = NULL, *d_iq = NULL, *d_pairs = NULL;
    float *h_pairs = NULL;
    size_t pairs_cap = 0;
    if (name == NULL || batch == NULL || batch_of == NULL) usage_error("out of memory");
    if (fsea_host_alloc(2 * BATCH_SAMPLES, &h_iq) != FSEA_OK) die("fsea_host_alloc");
    if (fsea_device_alloc(0, 2 * BATCH_SAMPLES, &d_iq) != FSEA_OK) die("fsea_device_alloc");
    for (size_t j = 0; j < n_jobs;) {
        /* a batch: the jobs from j on whose samples fit the buffer, back to back */
        size_t n_batch = 0, at = 0;
        for (; j < n_jobs && at + (size_t)jobs[j].n_samples <= BATCH_SAMPLES; j++) {
            if (jobs[j].n_samples == 0) continue;
            if (fseek(fp, (long)(2 * jobs[j].first), SEEK_SET) != 0 ||
                fread((uint8_t *)h_iq + 2 * at, 2, (size_t)jobs[j].n_samples, fp) != (size_t)jobs[j].n_samples) {
                fprintf(stderr, TOOL ": short read of %s\n", path);
                return EXIT_FAILURE;
            }
            batch[n_batch] = jobs[j];
            batch[n_batch].first = at;   /* its place in the buffer; sample_offset stays the stream position */
            batch_of[n_batch++] = j;
            at += (size_t)jobs[j].n_samples;
        }
        if (n_batch == 0) continue;
        size_t total = 0;
        if (fsea_extract_layout(extract, batch, n_batch, &total) != FSEA_OK) die("fsea_extract_layout");
        if (total == 0) continue;
        if (total > pairs_cap) {
            if (d_pairs != NULL) fsea_device_free(0, d_pairs);
            if (h_pairs != NULL) fsea_host_free(h_pairs);
            pairs_cap = total + total / 2;
            void *h = NULL;
            if (fsea_device_alloc(0, pairs_cap * 2 * sizeof(float), &d_pairs) != FSEA_OK) die("fsea_device_alloc");
            if (fsea_host_alloc(pairs_cap * 2 * sizeof(float), &h) != FSEA_OK) die("fsea_host_alloc");
            h_pairs = (float *)h;
        }
        if (fsea_copy_to_device(0, d_iq, h_iq, 2 * at) != FSEA_OK) die("fsea_copy_to_device");
        if (fsea_extract_run_device(extract, d_iq, at, flip, batch, n_batch, d_pairs, total, NULL) != FSEA_OK) die("fsea_extract_run_device");
        if (measures) {
            /* the spans the files get, on the pairs as they lie on the device */
            if (fsea_measure_jobs(batch, n_batch, decimation, lead_out, spans) != FSEA_OK) die("fsea_measure_jobs");
            if (fsea_measure_run_device(measure, d_pairs, total, spans, n_batch, pedestal, pedestal, lag, (fsea_measure_sums *)d_sums,
                                        NULL) != FSEA_OK) {
                die("fsea_measure_run_device");
            }
            if (fsea_copy_to_host(0, h_sums, d_sums, n_batch * sizeof(fsea_measure_sums)) != FSEA_OK) die("fsea_copy_to_host");
            for (size_t b = 0; b < n_batch; b++) {
                if (fsea_measure_finish(&h_sums[b], lag, &measured[batch_of[b]]) != FSEA_OK) die("fsea_measure_finish");
            }
        }
        size_t total_audio = 0;
        if (audio_kind >= 0) {
            /* the spans the files get, as the measures'; every span's audio back to back */
            if (fsea_measure_jobs(batch, n_batch, decimation, lead_out, audio_spans) != FSEA_OK) die("fsea_measure_jobs");
            for (size_t b = 0; b < n_batch; b++) {
                audio_jobs[b].first_pair = audio_spans[b].first_pair;
                audio_jobs[b].n_pairs = audio_spans[b].n_pairs;
                audio_jobs[b].out_first = 0;
            }
            if (fsea_audio_layout(audio, audio_jobs, n_batch, &total_audio) != FSEA_OK) die("fsea_audio_layout");
            if (total_audio > audio_cap) {
                if (d_audio != NULL) fsea_device_free(0, d_audio);
                if (h_audio != NULL) fsea_host_free(h_audio);
                audio_cap = total_audio + total_audio / 2;
                void *h = NULL;
                if (fsea_device_alloc(0, audio_cap * sizeof(float), &d_audio) != FSEA_OK) die("fsea_device_alloc");
                if (fsea_host_alloc(audio_cap * sizeof(float), &h) != FSEA_OK) die("fsea_host_alloc");
                h_audio = (float *)h;
            }
            if (total_audio > 0) {
                if (fsea_audio_run_device(audio, d_pairs, total, audio_jobs, n_batch, pedestal, pedestal, audio_gain, (float *)d_audio,
                                          total_audio, NULL) != FSEA_OK) {
                    die("fsea_audio_run_device");
                }
                if (fsea_copy_to_host(0, h_audio, d_audio, total_audio * sizeof(float)) != FSEA_OK) die("fsea_copy_to_host");
            }
        }
        if (fsea_copy_to_host(0, h_pairs, d_pairs, total * 2 * sizeof(float)) != FSEA_OK) die("fsea_copy_to_host");
        for (size_t b = 0; b < n_batch; b++) {
            const size_t n_out = (size_t)batch[b].n_samples / (size_t)decimation, e = batch_of[b];
            if (n_out <= lead_out) continue;
            snprintf(name, name_len, "%s/cutout-%05u.cf32", out_dir, (unsigned)e);
            FILE *out = fopen(name, "wb");
            const size_t keep = n_out - lead_out;
            if (out == NULL || fwrite(h_pairs + 2 * ((size_t)batch[b].out_first + lead_out), 2 * sizeof(float), keep, out) != keep ||
                fclose(out) != 0) {
                return cannot_write(name);
            }
            written[e] = keep;
            n_cutouts++;
            if (audio_kind >= 0) {
                const size_t n_audio = (size_t)audio_jobs[b].n_pairs / (size_t)audio_decimation;
                const float *a = h_audio + audio_jobs[b].out_first;
                if (n_audio == 0) continue;
                if (n_audio > pcm_cap) {
                    free(pcm);
                    pcm_cap = n_audio + n_audio / 2;
                    pcm = (int16_t *)malloc(sizeof(int16_t) * pcm_cap);
                    if (pcm == NULL) usage_error("out of memory");
                }
                double mean = 0.0, peak = 0.0;
                if (audio_kind == FSEA_AUDIO_AM) {   /* the carrier's level: the sum in order, over the count */
                    for (size_t i = 0; i < n_audio; i++) mean += (double)a[i];
                    mean /= (double)n_audio;
                }
                for (size_t i = 0; i < n_audio; i++) {
                    const double v = (double)a[i] - mean, s = v * 32000.0, mag = v < 0.0 ? -v : v;
                    if (mag > peak) peak = mag;
                    pcm[i] = s >= 32767.0 ? 32767 : s <= -32768.0 ? -32768 : s == s ? (int16_t)s : 0;
                }
                snprintf(name, name_len, "%s/cutout-%05u.wav", out_dir, (unsigned)e);
                if (write_wav(name, (uint32_t)(out_rate + 0.5), pcm, n_audio)) return cannot_write(name);
                fprintf(audio_list, "%u %.3f %zu %.6f\n", (unsigned)e, out_rate, n_audio, peak);
                n_audio_files++;
            }
        }
    }

    snprintf(name, name_len, "%s/cutouts.txt", out_dir);
    FILE *list = fopen(name, "w");
    if (list == NULL) return cannot_write(name);
    for (size_t e = 0; e < n_events; e++) {
        const fsea_events_event *ev = &found_events[e];
        const int listed = e < n_jobs;
        const double mhz = rate > 0.0 ? 0.5 * (tool_column_mhz(freq, rate, size, ev->col_first) + tool_column_mhz(freq, rate, size, ev->col_last)) : 0.0;
        fprintf(list, "%u %u %u %u %u %llu %llu %.6f %.3f %zu %d %d\n", (unsigned)e, ev->row_first, ev->row_last, ev->col_first,
                ev->col_last, listed ? (unsigned long long)jobs[e].first : 0ull, listed ? (unsigned long long)jobs[e].n_samples : 0ull, mhz,
                rate / (double)decimation, written[e], listed ? (int)fits[e] : 0, listed ? (int)cut[e] : 0);
    }
    if (fclose(list) != 0) return cannot_write(name);
    if (measures) {
        snprintf(name, name_len, "%s/measures.txt", out_dir);
        FILE *table = fopen(name, "w");
        if (table == NULL) return cannot_write(name);
        for (size_t e = 0; e < n_jobs; e++) {
            const fsea_measure_result *r = &measured[e];
            if (written[e] == 0) continue;
            fprintf(table, "%u %zu %.9e %.9e %.9e %.9e %.9e %.9e %.9e %.9e\n", (unsigned)e, written[e], r->power_db, r->freq_cycles,
                    r->freq_cycles * rate / (double)decimation / 1e6, r->width_cycles, r->kurtosis, r->crest, r->dc_re, r->dc_im);
        }
        if (fclose(table) != 0) return cannot_write(name);
        fsea_measure_destroy(measure);
        fsea_device_free(0, d_sums);
        free(measured);
        free(spans);
        free(h_sums);
    }
    if (audio_kind >= 0) {
        snprintf(name, name_len, "%s/audio.txt", out_dir);
        if (fclose(audio_list) != 0) return cannot_write(name);
        fsea_audio_destroy(audio);
        if (d_audio != NULL) fsea_device_free(0, d_audio);
        if (h_audio != NULL) fsea_host_free(h_audio);
        free(pcm);
        free(audio_spans);
        free(audio_jobs);
        printf("rows %zu runs %zu events %zu cutouts %zu skipped %zu audio %zu\n", done, runs.n, n_events, n_cutouts, n_events - n_cutouts,
               n_audio_files);
    } else {
        printf("rows %zu runs %zu events %zu cutouts %zu skipped %zu\n", done, runs.n, n_events, n_cutouts, n_events - n_cutouts);
    }

    fsea_extract_destroy(extract);
    fsea_events_destroy(events);
    fsea_cfar_destroy(cfar);
    fsea_device_free(0, d_iq);
    if (d_pairs != NULL) fsea_device_free(0, d_pairs);
    if (h_pairs != NULL) fsea_host_free(h_pairs);
    fsea_host_free(h_iq);
    fclose(fp);
    free(name);
    free(batch);
    free(batch_of);
    free(jobs);
    free(fits);
    free(cut);
    free(written);
    free(taps);
    free(found_events);
    free(runs.runs);
    return 0;
}
