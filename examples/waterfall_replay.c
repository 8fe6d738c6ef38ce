/* waterfall_replay.c -- the waterfall of an IQ capture, through nothing but the C ABI.
 *
 *     waterfall_replay CAPTURE OUT.f32 [--s16] [--n N] [--hop H] [--group G] [--reduce power|mag|max] [--db] [--window W] [--shift]
 *                      [--push SAMPLES]
 *
 * CAPTURE: interleaved unsigned 8-bit (I, Q) pairs (an RTL-SDR dump) or, with --s16, interleaved int16 pairs (a BladeRF dump).
 * Row r of the spectrum covers samples [r H, r H + N) (defaults N = 1024, H = N), windowed (--window none|hanning|hamming|blackman,
 * default hanning) and, with --shift, put DC in the middle (halfBandUp); output row R is the mean power, mean magnitude (the default)
 * or maximum over the G (default 1) consecutive rows R G .. R G + G - 1, linear or with --db in dB (never below -200).  The capture is
 * pushed SAMPLES (default 8192) at a time into a sdrhip_pipe_spectrum, read straight into its staging memory, the rest in one shorter
 * push; OUT.f32 receives the rows as raw float32, N per row.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdr_hip.h"

static void die(const char *what)
{
    fprintf(stderr, "waterfall_replay: %s: %s\n", what, sdrhip_last_error());
    exit(1);
}

static FILE *g_out;
static float *g_row;
static int g_n;
static long long g_rows;

static void drain(sdrhip_pipe *p, int ready)
{
    for (; ready > 0; ready--) {
        const int len = sdrhip_pipe_pop(p, g_row, g_n);
        if (len < 0) die("sdrhip_pipe_pop");
        if (len == 0) break;
        if (fwrite(g_row, sizeof(float), (size_t)len, g_out) != (size_t)len) { perror("write"); exit(1); }
        g_rows++;
    }
}

int main(int argc, char **argv)
{
    int n = 1024, group = 1, reduce = SDRHIP_REDUCE_MEAN_MAGNITUDE, unit = SDRHIP_UNIT_LINEAR, window = SDRHIP_WINDOW_HANNING;
    int shift = 0, s16 = 0, push = 8192;
    long long hop = 0;
    if (argc < 3) {
        fprintf(stderr, "usage: %s CAPTURE OUT.f32 [--s16] [--n N] [--hop H] [--group G] [--reduce power|mag|max] [--db] [--window W] [--shift] "
                        "[--push SAMPLES]\n", argv[0]);
        return 2;
    }
    for (int i = 3; i < argc; i += 2) {
        if (!strcmp(argv[i], "--s16")) { s16 = 1; i--; continue; }
        if (!strcmp(argv[i], "--db")) { unit = SDRHIP_UNIT_DB; i--; continue; }
        if (!strcmp(argv[i], "--shift")) { shift = 1; i--; continue; }
        if (i + 1 >= argc) { fprintf(stderr, "waterfall_replay: %s needs a value\n", argv[i]); return 2; }
        const char *v = argv[i + 1];
        if (!strcmp(argv[i], "--n")) n = atoi(v);
        else if (!strcmp(argv[i], "--hop")) hop = atoll(v);
        else if (!strcmp(argv[i], "--group")) group = atoi(v);
        else if (!strcmp(argv[i], "--push")) push = atoi(v);
        else if (!strcmp(argv[i], "--reduce")) {
            if (!strcmp(v, "power")) reduce = SDRHIP_REDUCE_MEAN_POWER;
            else if (!strcmp(v, "mag")) reduce = SDRHIP_REDUCE_MEAN_MAGNITUDE;
            else if (!strcmp(v, "max")) reduce = SDRHIP_REDUCE_MAX_MAGNITUDE;
            else { fprintf(stderr, "waterfall_replay: --reduce power|mag|max\n"); return 2; }
        } else if (!strcmp(argv[i], "--window")) {
            if (!strcmp(v, "none")) window = SDRHIP_WINDOW_NONE;
            else if (!strcmp(v, "hanning")) window = SDRHIP_WINDOW_HANNING;
            else if (!strcmp(v, "hamming")) window = SDRHIP_WINDOW_HAMMING;
            else if (!strcmp(v, "blackman")) window = SDRHIP_WINDOW_BLACKMAN;
            else { fprintf(stderr, "waterfall_replay: --window none|hanning|hamming|blackman\n"); return 2; }
        } else { fprintf(stderr, "waterfall_replay: unknown option %s\n", argv[i]); return 2; }
    }
    if (hop == 0) hop = n;
    if (n < 2 || push < 1) { fprintf(stderr, "waterfall_replay: --n >= 2, --push >= 1\n"); return 2; }

    sdrhip_spectrum *spec = NULL;
    if (sdrhip_spectrum_create(&spec, n, s16 ? SDRHIP_IQ_I16 : SDRHIP_IQ_U8, window, NULL, shift, 1.0) != SDRHIP_OK) die("sdrhip_spectrum_create");
    sdrhip_pipe *pipe = NULL;
    if (sdrhip_pipe_spectrum(&pipe, spec, hop, group, reduce, unit, -200.0) != SDRHIP_OK) die("sdrhip_pipe_spectrum");

    FILE *cap = fopen(argv[1], "rb");
    if (!cap) { perror(argv[1]); return 1; }
    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 1; }
    g_n = n;
    g_row = malloc(sizeof(float) * (size_t)n);
    if (!g_row) return 1;

    long long total = 0;
    for (;;) {
        /* read straight into the pinned staging memory of the next push */
        void *dst = s16 ? (void *)sdrhip_pipe_input_buffer_i16(pipe, push) : (void *)sdrhip_pipe_input_buffer_u8(pipe, push);
        if (!dst) die("sdrhip_pipe_input_buffer");
        const int got = (int)fread(dst, s16 ? 4 : 2, (size_t)push, cap);
        if (got < 1) break;
        const int ready = s16 ? sdrhip_pipe_push_i16(pipe, dst, got) : sdrhip_pipe_push_u8(pipe, dst, got);
        if (ready < 0) die("sdrhip_pipe_push");
        drain(pipe, ready);
        total += got;
        if (got < push) break;
    }
    const int ready = sdrhip_pipe_flush(pipe);
    if (ready < 0) die("sdrhip_pipe_flush");
    drain(pipe, ready);

    fprintf(stderr, "waterfall_replay: %lld samples in, n %d, hop %lld, group %d, %lld rows out\n", total, n, hop, group, g_rows);
    fclose(g_out);
    fclose(cap);
    free(g_row);
    sdrhip_pipe_destroy(pipe);
    sdrhip_spectrum_destroy(spec);
    return 0;
}
