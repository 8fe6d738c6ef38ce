/* squelch_scan.c -- a scanner's inner step: every narrow channel of one u8 IQ capture demodulated and squelched on the device, through
 * nothing but the C ABI.
 *
 *     squelch_scan CAPTURE.u8 TAPS.f32 OUT_PREFIX --channels NUM/DEN[,NUM/DEN...] --narrow TAPS2.f32 D2 --form fm|env
 *                  --squelch OPEN,CLOSE,HANG --block N [--factor D]
 *
 * CAPTURE.u8: interleaved unsigned 8-bit (I, Q) pairs.  TAPS.f32 / TAPS2.f32: the coefficients of the first decimator (factor D,
 * default 8) and of the second (factor D2), raw float32.  Channel j is the capture shifted by NUM/DEN cycles per sample.  The whole
 * capture is uploaded once; ONE sdrhip_narrow_bank_run_u8 gives every channel's demodulated row (fmDemod from (0, 0) with --form fm,
 * the envelope with --form env), and ONE sdrhip_squelch_run_rows gates all rows in place, each row its own detector, in blocks of N
 * samples from the state {0, 0}: with fm the gate opens where the block's mean square is at or BELOW OPEN and shuts above CLOSE (a
 * quieting squelch: the phase of a channel without a carrier is full-scale noise), with env it opens at or ABOVE OPEN and shuts below
 * CLOSE (a carrier squelch on the envelope); HANG blocks behind the last open one stay open.  Only whole blocks are written:
 * OUT_PREFIX.<j>.f32 holds channel j's gated samples as float32, OUT_PREFIX.<j>.gate one byte (0 / 1) per block.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdr_hip.h"

#define MAX_CH SDRHIP_TUNER_BANK_MAX_CHANNELS

static void die(const char *what)
{
    fprintf(stderr, "squelch_scan: %s: %s\n", what, sdrhip_last_error());
    exit(1);
}

static int usage(const char *why)
{
    fprintf(stderr, "squelch_scan: %s\nusage: squelch_scan CAPTURE.u8 TAPS.f32 OUT_PREFIX --channels NUM/DEN[,...] --narrow TAPS2.f32 D2 "
                    "--form fm|env --squelch OPEN,CLOSE,HANG --block N [--factor D]\n", why);
    return 2;
}

static void *read_file(const char *path, size_t *bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(1); }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    void *v = malloc(n > 0 ? (size_t)n : 1);
    if (!v || fread(v, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "squelch_scan: cannot read %s\n", path); exit(1); }
    fclose(f);
    *bytes = (size_t)n;
    return v;
}

static void write_file(const char *prefix, int j, const char *ext, const void *data, size_t bytes)
{
    char name[4096];
    snprintf(name, sizeof name, "%s.%d.%s", prefix, j, ext);
    FILE *f = fopen(name, "wb");
    if (!f || fwrite(data, 1, bytes, f) != bytes) { perror(name); exit(1); }
    fclose(f);
}

int main(int argc, char **argv)
{
    const char *spec = NULL, *narrow_path = NULL, *form_name = NULL, *squelch = NULL;
    int factor = 8, factor2 = 0, block = 0;
    if (argc < 4) return usage("too few arguments");
    for (int i = 4; i < argc; i += 2) {
        if (!strcmp(argv[i], "--narrow")) {
            if (i + 2 >= argc) return usage("--narrow needs TAPS2.f32 D2");
            narrow_path = argv[i + 1];
            factor2 = atoi(argv[i + 2]);
            i++;
            continue;
        }
        if (i + 1 >= argc) return usage("an option needs a value");
        if (!strcmp(argv[i], "--channels")) spec = argv[i + 1];
        else if (!strcmp(argv[i], "--factor")) factor = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--form")) form_name = argv[i + 1];
        else if (!strcmp(argv[i], "--squelch")) squelch = argv[i + 1];
        else if (!strcmp(argv[i], "--block")) block = atoi(argv[i + 1]);
        else return usage("unknown option");
    }
    float open_level = 0.0f, close_level = 0.0f;
    int hang = 0;
    if (!spec || !narrow_path || !form_name || !squelch) return usage("--channels, --narrow, --form and --squelch are required");
    if (strcmp(form_name, "fm") && strcmp(form_name, "env")) return usage("--form fm|env");
    if (sscanf(squelch, "%f,%f,%d", &open_level, &close_level, &hang) != 3) return usage("--squelch OPEN,CLOSE,HANG");
    if (factor < 1 || factor2 < 1 || block < 1) return usage("--factor, D2 and --block are positive");
    const int fm = !strcmp(form_name, "fm");

    float *tables[MAX_CH];
    int periods[MAX_CH], channels = 0;
    for (const char *s = spec; *s;) {
        long long num, den;
        int used = 0;
        if (channels == MAX_CH || sscanf(s, "%lld/%lld%n", &num, &den, &used) != 2 || den < 1 || den > 65536) return usage("bad channel list");
        tables[channels] = malloc(sizeof(float) * 2 * (size_t)den);
        if (!tables[channels]) return 1;
        if (sdrhip_tuner_shift_table(num, den, tables[channels]) != SDRHIP_OK) die("sdrhip_tuner_shift_table");
        periods[channels++] = (int)den;
        s += used;
        if (*s == ',') s++;
    }

    size_t cap_bytes = 0, t1_bytes = 0, t2_bytes = 0;
    uint8_t *cap = read_file(argv[1], &cap_bytes);
    float *taps = read_file(argv[2], &t1_bytes), *taps2 = read_file(narrow_path, &t2_bytes);
    sdrhip_tuner_bank *bank = NULL;
    sdrhip_decimator *deci2 = NULL;
    sdrhip_narrow_bank *narrow = NULL;
    if (sdrhip_tuner_bank_create(&bank, 2 /* the AVX order */, factor, taps, (int)(t1_bytes / 4), channels, (const float *const *)tables, periods) != SDRHIP_OK)
        die("sdrhip_tuner_bank_create");
    if (sdrhip_decimator_create(&deci2, 2 /* the AVX order */, 1 /* complex data */, factor2, taps2, (int)(t2_bytes / 4)) != SDRHIP_OK)
        die("sdrhip_decimator_create");
    if (sdrhip_narrow_bank_create(&narrow, bank, deci2, fm ? SDRHIP_NARROW_FM : SDRHIP_NARROW_ENV, 0) != SDRHIP_OK) die("sdrhip_narrow_bank_create");

    /* the whole blocks the capture gives: N samples -> J stage-1 outputs -> K stage-2 outputs -> K / block blocks */
    const int64_t n = (int64_t)(cap_bytes / 2);
    const int64_t lp1 = sdrhip_tuner_bank_num_coeffs(bank), lp2 = sdrhip_decimator_num_coeffs(deci2);
    const int64_t j_all = n >= lp1 ? (n - lp1) / factor + 1 : 0;
    const int64_t k_all = j_all >= lp2 ? (j_all - lp2) / factor2 + 1 : 0;
    const int64_t n_blocks = k_all / block, count = n_blocks * block;
    if (n_blocks < 1) { fprintf(stderr, "squelch_scan: the capture gives %lld samples a channel, less than one block of %d\n", (long long)k_all, block); return 1; }

    void *d_cap = NULL, *d_rows = NULL, *d_gates = NULL, *d_ws = NULL, *d_sq_ws = NULL;
    const size_t row_bytes = sizeof(float) * (size_t)count, ws_bytes = sdrhip_narrow_bank_workspace_bytes(narrow, count);
    const size_t sq_ws_bytes = sdrhip_squelch_rows_workspace_bytes(channels, n_blocks);
    if (ws_bytes == 0) die("sdrhip_narrow_bank_workspace_bytes");
    if (sdrhip_malloc(&d_cap, cap_bytes) != SDRHIP_OK || sdrhip_malloc(&d_rows, row_bytes * (size_t)channels) != SDRHIP_OK ||
        sdrhip_malloc(&d_gates, (size_t)channels * (size_t)n_blocks) != SDRHIP_OK || sdrhip_malloc(&d_ws, ws_bytes) != SDRHIP_OK ||
        sdrhip_malloc(&d_sq_ws, sq_ws_bytes) != SDRHIP_OK)
        die("sdrhip_malloc");
    if (sdrhip_memcpy_h2d(d_cap, cap, cap_bytes, NULL) != SDRHIP_OK) die("sdrhip_memcpy_h2d");
    if (sdrhip_narrow_bank_run_u8(narrow, NULL, d_cap, 0, d_rows, count, 0, count, 0, 0, NULL, NULL, NULL, d_ws, ws_bytes) != SDRHIP_OK)
        die("sdrhip_narrow_bank_run_u8");
    /* every row is its own detector and is gated in place */
    if (sdrhip_squelch_run_rows(NULL, d_rows, count, 0, block, d_rows, count, d_rows, count, block, channels, n_blocks, open_level, close_level,
                                hang, fm ? 0 : 1, NULL, NULL, NULL, d_gates, d_sq_ws, sq_ws_bytes) != SDRHIP_OK)
        die("sdrhip_squelch_run_rows");

    float *rows = malloc(row_bytes * (size_t)channels);
    uint8_t *gates = malloc((size_t)channels * (size_t)n_blocks);
    if (!rows || !gates) return 1;
    if (sdrhip_memcpy_d2h(rows, d_rows, row_bytes * (size_t)channels, NULL) != SDRHIP_OK) die("sdrhip_memcpy_d2h");
    if (sdrhip_memcpy_d2h(gates, d_gates, (size_t)channels * (size_t)n_blocks, NULL) != SDRHIP_OK) die("sdrhip_memcpy_d2h");
    if (sdrhip_stream_sync(NULL) != SDRHIP_OK) die("sdrhip_stream_sync");
    long long open_blocks = 0;
    for (int j = 0; j < channels; j++) {
        write_file(argv[3], j, "f32", rows + (size_t)j * (size_t)count, row_bytes);
        write_file(argv[3], j, "gate", gates + (size_t)j * (size_t)n_blocks, (size_t)n_blocks);
        for (int64_t b = 0; b < n_blocks; b++) open_blocks += gates[(size_t)j * (size_t)n_blocks + (size_t)b];
    }
    fprintf(stderr, "squelch_scan: %lld samples, %d channels, %lld blocks of %d a channel, %lld open\n", (long long)n, channels,
            (long long)n_blocks, block, open_blocks);

    free(rows); free(gates); free(cap); free(taps); free(taps2);
    for (int j = 0; j < channels; j++) free(tables[j]);
    sdrhip_free(d_cap); sdrhip_free(d_rows); sdrhip_free(d_gates); sdrhip_free(d_ws); sdrhip_free(d_sq_ws);
    sdrhip_narrow_bank_destroy(narrow);
    sdrhip_decimator_destroy(deci2);
    sdrhip_tuner_bank_destroy(bank);
    return 0;
}
