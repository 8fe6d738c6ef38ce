/* nfm_replay.c -- the narrow-band FM demodulator for every channel of one u8 or int16 IQ capture, through nothing but the C ABI.
 *
 *     nfm_replay CAPTURE TAPS.f32 OUT_PREFIX --channels NUM/DEN[,NUM/DEN...] [--factor D] [--block-out N] [--push SAMPLES] [--s16]
 *                [--audio RESAMP_TAPS.f32 AUDIO_HALF_TAPS.f32 [--ratio I/D] [--gain G]]
 *                [--narrow TAPS2.f32 D2 [--block-mid N]]
 *
 * CAPTURE: interleaved unsigned 8-bit (I, Q) pairs (an RTL-SDR dump); with --s16 interleaved signed 16-bit pairs in host byte order (a
 * BladeRF dump).  TAPS.f32: the decimator's coefficients, raw float32.  Channel j is the capture shifted by NUM/DEN cycles per sample
 * (sdrhip_tuner_shift_table; 0/1 is the centre frequency), decimated by D (default 8) and put through fmDemod from (0, 0); its
 * demodulated samples go to OUT_PREFIX.chJ.f32 as float32, whole blocks of N (default 1024) only, as the Pipe yields them.  The
 * capture is pushed SAMPLES (default 8192) at a time, the rest in one shorter push.  ONE Pipe for all channels (sdrhip_pipe_nfm_bank
 * over sdrhip_nfm_bank over sdrhip_tuner_bank): one copy over the link per push, K float rows back.  What follows the demodulator
 * in a receiver is the caller's (de-emphasis: sdrhip_deemph_run_rows; squelch: sdrhip_squelch_run_rows, as examples/squelch_scan.c
 * uses it); a second decimator in FRONT of the demodulator is --narrow, below.
 * With --audio the files hold AUDIO instead: the demodulated samples resampled by I/D (default 3/10: 160 ksample/s to 48 k) with the
 * taps of RESAMP_TAPS.f32, filtered with the symmetric filter whose first half is AUDIO_HALF_TAPS.f32 and multiplied by G (default
 * 1), every Pipe of those stages with blocks of N -- sdrhip_pipe_nfm_bank_audio over an sdrhip_audio_tail, still ONE Pipe, one copy
 * over the link per push and K audio rows back.
 * With --narrow the files hold the NARROW channel instead: a second complex decimator by D2 with the coefficients of TAPS2.f32 between
 * the first decimator and the demodulator -- firDecimator deci1 N_mid >-> firDecimator deci2 N >-> demodulator, N_mid from --block-mid
 * (default 1024 stage-1 outputs) -- as ONE Pipe still: sdrhip_pipe_narrow_bank over sdrhip_narrow_bank.  --narrow excludes --audio.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdr_hip.h"

#define MAX_CH SDRHIP_TUNER_BANK_MAX_CHANNELS

static void die(const char *what)
{
    fprintf(stderr, "nfm_replay: %s: %s\n", what, sdrhip_last_error());
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
    if (!v || fread(v, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "nfm_replay: cannot read %s\n", path); exit(1); }
    fclose(f);
    *n = (int)(bytes / 4);
    return v;
}

/* every ready block of every channel: rows[j] holds nb blocks, appended to file j */
static void drain(sdrhip_pipe *p, int ready, int channels, int block_out, float *rows, FILE **out)
{
    while (ready > 0) {
        const int want = ready < 16 ? ready : 16;
        const int64_t stride = (int64_t)16 * block_out;
        const int nb = sdrhip_pipe_pop_rows(p, rows, stride, want);
        if (nb < 0) die("sdrhip_pipe_pop_rows");
        if (nb == 0) break;
        for (int j = 0; j < channels; j++)
            if (fwrite(rows + j * stride, sizeof(float), (size_t)nb * block_out, out[j]) != (size_t)nb * block_out) {
                perror("write");
                exit(1);
            }
        ready -= nb;
    }
}

int main(int argc, char **argv)
{
    const char *spec = NULL;
    const char *resamp_path = NULL, *audio_path = NULL, *narrow_path = NULL;
    int factor2 = 0, block_mid = 1024;
    int factor = 8, block_out = 1024, push = 8192, s16 = 0, interp = 3, decim = 10;
    float gain = 1.0f;
    if (argc < 4) {
        fprintf(stderr, "usage: %s CAPTURE.u8 TAPS.f32 OUT_PREFIX --channels NUM/DEN[,...] [--factor D] [--block-out N] [--push SAMPLES] [--s16]\n", argv[0]);
        return 2;
    }
    for (int i = 4; i < argc; i += 2) {
        if (!strcmp(argv[i], "--s16")) { s16 = 1; i--; continue; }
        if (!strcmp(argv[i], "--audio")) {
            if (i + 2 >= argc) { fprintf(stderr, "nfm_replay: --audio needs RESAMP_TAPS.f32 AUDIO_HALF_TAPS.f32\n"); return 2; }
            resamp_path = argv[i + 1];
            audio_path = argv[i + 2];
            i++;
            continue;
        }
        if (!strcmp(argv[i], "--narrow")) {
            if (i + 2 >= argc) { fprintf(stderr, "nfm_replay: --narrow needs TAPS2.f32 D2\n"); return 2; }
            narrow_path = argv[i + 1];
            factor2 = atoi(argv[i + 2]);
            i++;
            continue;
        }
        if (i + 1 >= argc) { fprintf(stderr, "nfm_replay: %s needs a value\n", argv[i]); return 2; }
        if (!strcmp(argv[i], "--channels")) spec = argv[i + 1];
        else if (!strcmp(argv[i], "--factor")) factor = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--block-out")) block_out = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--push")) push = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--block-mid")) block_mid = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--gain")) gain = (float)atof(argv[i + 1]);
        else if (!strcmp(argv[i], "--ratio")) {
            if (sscanf(argv[i + 1], "%d/%d", &interp, &decim) != 2) { fprintf(stderr, "nfm_replay: --ratio I/D\n"); return 2; }
        }
        else { fprintf(stderr, "nfm_replay: unknown option %s\n", argv[i]); return 2; }
    }
    if (!spec || factor < 1 || block_out < 1 || push < 1) { fprintf(stderr, "nfm_replay: --channels NUM/DEN[,...] is required\n"); return 2; }

    if (narrow_path && (resamp_path || factor2 < 1 || block_mid < 1)) {
        fprintf(stderr, "nfm_replay: --narrow TAPS2.f32 D2 [--block-mid N], without --audio\n");
        return 2;
    }

    /* the channels' shift tables */
    float *tables[MAX_CH];
    int periods[MAX_CH], channels = 0;
    for (const char *s = spec; *s;) {
        long long num, den;
        int used = 0;
        if (channels == MAX_CH || sscanf(s, "%lld/%lld%n", &num, &den, &used) != 2 || den < 1 || den > 65536) {
            fprintf(stderr, "nfm_replay: bad channel list at '%s' (NUM/DEN, DEN 1 .. 65536, at most %d channels)\n", s, MAX_CH);
            return 2;
        }
        tables[channels] = malloc(sizeof(float) * 2 * (size_t)den);
        if (!tables[channels]) return 1;
        if (sdrhip_tuner_shift_table(num, den, tables[channels]) != SDRHIP_OK) die("sdrhip_tuner_shift_table");
        periods[channels++] = (int)den;
        s += used;
        if (*s == ',') s++;
    }

    int ntaps = 0;
    float *taps = read_floats(argv[2], &ntaps);
    sdrhip_tuner_bank *bank = NULL;
    if (sdrhip_tuner_bank_create(&bank, 2 /* the AVX order */, factor, taps, ntaps, channels, (const float *const *)tables, periods) != SDRHIP_OK)
        die("sdrhip_tuner_bank_create");
    sdrhip_nfm_bank *nfm = NULL;
    if (sdrhip_nfm_bank_create(&nfm, bank) != SDRHIP_OK) die("sdrhip_nfm_bank_create");
    sdrhip_pipe *pipe = NULL;
    sdrhip_audio_tail *tail = NULL;
    sdrhip_decimator *deci2 = NULL;
    sdrhip_narrow_bank *narrow = NULL;
    if (narrow_path) {
        int nt2 = 0;
        float *t2 = read_floats(narrow_path, &nt2);
        if (sdrhip_decimator_create(&deci2, 2 /* the AVX order */, 1 /* complex data */, factor2, t2, nt2) != SDRHIP_OK) die("sdrhip_decimator_create");
        free(t2);
        if (sdrhip_narrow_bank_create(&narrow, bank, deci2, SDRHIP_NARROW_FM, 0) != SDRHIP_OK) die("sdrhip_narrow_bank_create");
        if (sdrhip_pipe_narrow_bank(&pipe, narrow, block_mid, block_out, s16 ? 2 : 1) != SDRHIP_OK) die("sdrhip_pipe_narrow_bank");
    } else if (resamp_path) {
        int nr = 0, na = 0;
        float *rt = read_floats(resamp_path, &nr), *ah = read_floats(audio_path, &na);
        if (sdrhip_audio_tail_create(&tail, 2 /* the AVX order */, interp, decim, rt, nr, ah, na, gain, block_out) != SDRHIP_OK)
            die("sdrhip_audio_tail_create");
        free(rt);
        free(ah);
        if (sdrhip_pipe_nfm_bank_audio(&pipe, nfm, tail, s16 ? 2 : 1) != SDRHIP_OK) die("sdrhip_pipe_nfm_bank_audio");
    } else if (sdrhip_pipe_nfm_bank(&pipe, nfm, block_out, s16 ? 2 : 1) != SDRHIP_OK) die("sdrhip_pipe_nfm_bank");

    FILE *cap = fopen(argv[1], "rb");
    if (!cap) { perror(argv[1]); return 1; }
    FILE *out[MAX_CH];
    for (int j = 0; j < channels; j++) {
        char name[4096];
        snprintf(name, sizeof name, "%s.ch%d.f32", argv[3], j);
        out[j] = fopen(name, "wb");
        if (!out[j]) { perror(name); return 1; }
    }
    float *rows = malloc(sizeof(float) * (size_t)channels * 16 * (size_t)block_out);
    if (!rows) return 1;

    const int lp = sdrhip_tuner_bank_num_coeffs(bank);
    long long total = 0;
    for (;;) {
        /* read straight into the pinned staging memory of the next push */
        void *dst = s16 ? (void *)sdrhip_pipe_input_buffer_i16(pipe, push) : (void *)sdrhip_pipe_input_buffer_u8(pipe, push);
        if (!dst) die(s16 ? "sdrhip_pipe_input_buffer_i16" : "sdrhip_pipe_input_buffer_u8");
        const int n = (int)(fread(dst, s16 ? 4 : 2, (size_t)push, cap));
        if (n < lp) break;                    /* the end of the capture: a rest shorter than the filter computes nothing */
        const int ready = s16 ? sdrhip_pipe_push_i16(pipe, (const int16_t *)dst, n) : sdrhip_pipe_push_u8(pipe, (const uint8_t *)dst, n);
        if (ready < 0) die(s16 ? "sdrhip_pipe_push_i16" : "sdrhip_pipe_push_u8");
        drain(pipe, ready, channels, block_out, rows, out);
        total += n;
        if (n < push) break;
    }
    const int ready = sdrhip_pipe_flush(pipe);
    if (ready < 0) die("sdrhip_pipe_flush");
    drain(pipe, ready, channels, block_out, rows, out);

    fprintf(stderr, "nfm_replay: %lld samples, %d channels, decimation %d\n", total, channels, factor);
    for (int j = 0; j < channels; j++) { fclose(out[j]); free(tables[j]); }
    fclose(cap);
    free(rows);
    free(taps);
    sdrhip_pipe_destroy(pipe);
    sdrhip_audio_tail_destroy(tail);
    sdrhip_narrow_bank_destroy(narrow);
    sdrhip_decimator_destroy(deci2);
    sdrhip_nfm_bank_destroy(nfm);
    sdrhip_tuner_bank_destroy(bank);
    return 0;
}
