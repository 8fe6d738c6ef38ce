/* am_replay.c -- an AM receiver for one channel of a u8 IQ capture, through nothing but the C ABI.
 *
 *     am_replay CAPTURE.u8 TAPS.f32 OUT.f32 --channel NUM/DEN [--factor D] [--block-out N] [--push SAMPLES] [--no-dc]
 *
 * CAPTURE.u8: interleaved unsigned 8-bit (I, Q) pairs (an RTL-SDR dump).  TAPS.f32: the decimator's coefficients, raw float32.
 * The capture is shifted by NUM/DEN cycles per sample (sdrhip_tuner_shift_table; 0/1 is the centre frequency) and decimated by D
 * (default 8) in blocks of N (default 1024) samples: a one-channel sdrhip_pipe_tuner_bank fed u8 blocks.  Every block then goes
 * through the envelope detector (sdrhip_pipe_am_demod: Data.Complex.magnitude of each sample) and, unless --no-dc is given, the
 * reference's dcBlockingFilter (sdrhip_pipe_dc_blocker), which takes the carrier out.  OUT.f32 receives the result as raw float32.
 * The capture is pushed SAMPLES (default 8192) at a time, the rest in one shorter push.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdr_hip.h"

static void die(const char *what)
{
    fprintf(stderr, "am_replay: %s: %s\n", what, sdrhip_last_error());
    exit(1);
}

static float *read_floats(const char *path, int *n)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(1); }
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    float *v = malloc(bytes > 0 ? (size_t)bytes : 1);
    if (!v || fread(v, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "am_replay: cannot read %s\n", path); exit(1); }
    fclose(f);
    *n = (int)(bytes / 4);
    return v;
}

static sdrhip_pipe *g_am, *g_dc;   /* g_dc is NULL with --no-dc */
static FILE *g_out;
static float *g_iq, *g_env, *g_audio;   /* one block each: block_out complex samples, block_out floats twice */
static int g_block;
static long long g_written;

/* `ready` blocks of the dcBlocker (or, without it, of the detector) to the file */
static void drain_last(sdrhip_pipe *p, float *buf, int ready)
{
    for (; ready > 0; ready--) {
        const int len = sdrhip_pipe_pop(p, buf, g_block);
        if (len < 0) die("sdrhip_pipe_pop");
        if (len == 0) break;
        if (fwrite(buf, sizeof(float), (size_t)len, g_out) != (size_t)len) { perror("write"); exit(1); }
        g_written += len;
    }
}

/* `ready` blocks of the detector into the dcBlocker */
static void drain_am(int ready)
{
    if (!g_dc) { drain_last(g_am, g_env, ready); return; }
    for (; ready > 0; ready--) {
        const int len = sdrhip_pipe_pop(g_am, g_env, g_block);
        if (len < 0) die("sdrhip_pipe_pop");
        if (len == 0) break;
        const int r = sdrhip_pipe_push(g_dc, g_env, len);
        if (r < 0) die("sdrhip_pipe_push (dcBlockingFilter)");
        drain_last(g_dc, g_audio, r);
    }
}

/* `ready` blocks of the tuner into the detector */
static void drain_tuner(sdrhip_pipe *tuner, int ready)
{
    for (; ready > 0; ready--) {
        const int len = sdrhip_pipe_pop(tuner, g_iq, g_block);
        if (len < 0) die("sdrhip_pipe_pop");
        if (len == 0) break;
        const int r = sdrhip_pipe_push(g_am, g_iq, len);
        if (r < 0) die("sdrhip_pipe_push (amDemod)");
        drain_am(r);
    }
}

int main(int argc, char **argv)
{
    const char *spec = NULL;
    int factor = 8, block_out = 1024, push = 8192, no_dc = 0;
    if (argc < 4) {
        fprintf(stderr, "usage: %s CAPTURE.u8 TAPS.f32 OUT.f32 --channel NUM/DEN [--factor D] [--block-out N] [--push SAMPLES] [--no-dc]\n", argv[0]);
        return 2;
    }
    for (int i = 4; i < argc; i += 2) {
        if (!strcmp(argv[i], "--no-dc")) { no_dc = 1; i--; continue; }
        if (i + 1 >= argc) { fprintf(stderr, "am_replay: %s needs a value\n", argv[i]); return 2; }
        if (!strcmp(argv[i], "--channel")) spec = argv[i + 1];
        else if (!strcmp(argv[i], "--factor")) factor = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--block-out")) block_out = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--push")) push = atoi(argv[i + 1]);
        else { fprintf(stderr, "am_replay: unknown option %s\n", argv[i]); return 2; }
    }
    long long num = 0, den = 0;
    if (!spec || sscanf(spec, "%lld/%lld", &num, &den) != 2 || den < 1 || den > 65536 || factor < 1 || block_out < 1 || push < 1) {
        fprintf(stderr, "am_replay: --channel NUM/DEN is required (DEN 1 .. 65536)\n");
        return 2;
    }

    float *table = malloc(sizeof(float) * 2 * (size_t)den);
    if (!table) return 1;
    if (sdrhip_tuner_shift_table(num, den, table) != SDRHIP_OK) die("sdrhip_tuner_shift_table");
    const float *tables[1] = {table};
    const int periods[1] = {(int)den};
    int ntaps = 0;
    float *taps = read_floats(argv[2], &ntaps);
    sdrhip_tuner_bank *bank = NULL;
    if (sdrhip_tuner_bank_create(&bank, 2 /* the AVX order */, factor, taps, ntaps, 1, (const float *const *)tables, periods) != SDRHIP_OK)
        die("sdrhip_tuner_bank_create");
    sdrhip_pipe *tuner = NULL;
    if (sdrhip_pipe_tuner_bank(&tuner, bank, block_out, 1) != SDRHIP_OK) die("sdrhip_pipe_tuner_bank");
    if (sdrhip_pipe_am_demod(&g_am) != SDRHIP_OK) die("sdrhip_pipe_am_demod");
    if (!no_dc && sdrhip_pipe_dc_blocker(&g_dc) != SDRHIP_OK) die("sdrhip_pipe_dc_blocker");

    FILE *cap = fopen(argv[1], "rb");
    if (!cap) { perror(argv[1]); return 1; }
    g_out = fopen(argv[3], "wb");
    if (!g_out) { perror(argv[3]); return 1; }
    g_block = block_out;
    g_iq = malloc(sizeof(float) * 2 * (size_t)block_out);
    g_env = malloc(sizeof(float) * (size_t)block_out);
    g_audio = malloc(sizeof(float) * (size_t)block_out);
    if (!g_iq || !g_env || !g_audio) return 1;

    const int lp = sdrhip_tuner_bank_num_coeffs(bank);
    long long total = 0;
    for (;;) {
        /* read straight into the pinned staging memory of the next push */
        uint8_t *dst = sdrhip_pipe_input_buffer_u8(tuner, push);
        if (!dst) die("sdrhip_pipe_input_buffer_u8");
        const int n = (int)fread(dst, 2, (size_t)push, cap);
        if (n < lp) break;                    /* the end of the capture: a rest shorter than the filter computes nothing */
        const int ready = sdrhip_pipe_push_u8(tuner, dst, n);
        if (ready < 0) die("sdrhip_pipe_push_u8");
        drain_tuner(tuner, ready);
        total += n;
        if (n < push) break;
    }
    /* the stages run dry one after the other: what a flush hands over goes into the next stage before that one is flushed */
    int ready = sdrhip_pipe_flush(tuner);
    if (ready < 0) die("sdrhip_pipe_flush");
    drain_tuner(tuner, ready);
    if ((ready = sdrhip_pipe_flush(g_am)) < 0) die("sdrhip_pipe_flush");
    drain_am(ready);
    if (g_dc) {
        if ((ready = sdrhip_pipe_flush(g_dc)) < 0) die("sdrhip_pipe_flush");
        drain_last(g_dc, g_audio, ready);
    }

    fprintf(stderr, "am_replay: %lld samples in, decimation %d, %lld floats out%s\n", total, factor, g_written, no_dc ? " (no dcBlockingFilter)" : "");
    fclose(g_out);
    fclose(cap);
    free(g_iq); free(g_env); free(g_audio); free(taps); free(table);
    if (g_dc) sdrhip_pipe_destroy(g_dc);
    sdrhip_pipe_destroy(g_am);
    sdrhip_pipe_destroy(tuner);
    sdrhip_tuner_bank_destroy(bank);
    return 0;
}
