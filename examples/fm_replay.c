/* fm_replay.c -- the FM receiver of the reference's examples/fm/fm.hs:30-41 fed from a file instead of a radio
 * ("file replay source feeding pinned buffers"), in plain C over the C ABI of libsdr_hip.so.
 *
 *     fm_replay [--s16] [--shift NUM/DEN | --stations NUM/DEN[,NUM/DEN...]] [--deemph TAU_US --audio-rate HZ]
 *               <iq_file | udp:PORT> <audio_f32_file> [blocks_per_push] [taps_prefix]
 *
 * Reads interleaved unsigned 8-bit IQ (what rtl_sdr writes, what RTLSDRStream.hs:48-67 yields) in source blocks of
 * 8192 samples, `blocks_per_push` of them at a time, straight into the stream operator's pinned staging buffer
 * (fread is the "source that can write where it is told"), and writes the audio blocks (8192 floats each, 48 kHz for
 * a 1.28 MHz capture) as raw little-endian f32.  With `udp:PORT` the samples come from UDP datagrams on 127.0.0.1:PORT
 * instead (the reference's udpSource, NetworkStream.hs:28-35), reassembled into source blocks; a zero-length datagram
 * ends the stream.  Taps arrive as three raw f32 files (<taps_prefix>.decim.f32, .resamp.f32, .audio_half.f32; the
 * prefix defaults to the capture's path) so the example carries no filter design of its own.
 * --shift NUM/DEN receives a station that is off the centre of the capture: the samples are multiplied by exp(2 pi i NUM n / DEN)
 * (sdrhip_tuner_shift_table, 1 <= DEN <= 65536; sample n of the capture meets entry n mod DEN) in front of the decimator
 * (sdrhip_fm_chain_set_tuner), which moves the station NUM / DEN of the sampling frequency BELOW the centre onto it.
 * --stations NUM/DEN[,NUM/DEN...] receives 1 to 32 stations of the capture at once: one table per station (sdrhip_tuner_shift_table),
 * ONE bank (sdrhip_fm_bank_create), ONE stream over it (sdrhip_fm_stream_create_bank) -- every push crosses the link once and is one
 * launch for all the stations.  Station j's audio goes to <audio_f32_file>.<j> and is what --shift with its NUM/DEN writes.
 * --s16: the capture is interleaved signed 16-bit IQ (a BladeRF's samples, s / 2048), 4 bytes per sample.  16-bit input reaches the
 * FM side through a bank, so the receiver is then always a bank and an int16 stream over it (sdrhip_fm_stream_create_bank_i16,
 * sdrhip_fm_stream_push_i16): the --stations given, or ONE station -- the --shift table, or {1, 0} when neither is given, which is
 * the plain receiver (a converted int16 sample times 1 + 0i keeps its bits) -- whose audio goes to <audio_f32_file> itself.
 * --deemph TAU_US --audio-rate HZ (both or neither): the popped audio blocks of every station go through a de-emphasis Pipe
 * (sdrhip_pipe_deemph, alpha = sdrhip_deemph_alpha(TAU_US * 1e-6, HZ); 75 us in the Americas, 50 us elsewhere; 48000 Hz for a 1.28 MHz
 * capture), one Pipe per station, chained behind the stream the way am_replay.c chains its Pipes.  Without the flags nothing changes.
 * Output is bit-identical to the reference pipeline's (tests/test_gpu_examples.py); with --deemph, to tests/deemph_model.py on it. */
#define _POSIX_C_SOURCE 200809L
#include <arpa/inet.h>
#include <netinet/in.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/time.h>
#include <unistd.h>

#include "sdr_hip.h"

#define SOURCE_BLOCK 8192 /* fm.hs:17 `samples` */

static float *read_floats(const char *base, const char *suffix, int *n)
{
    char path[4096];
    snprintf(path, sizeof path, "%s%s", base, suffix);
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "fm_replay: cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    float *v = (float *)malloc((size_t)bytes);
    if (fread(v, 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "fm_replay: short read on %s\n", path); exit(2); }
    fclose(f);
    *n = (int)(bytes / 4);
    return v;
}

/* The sample source: a file, or a UDP socket whose datagrams are concatenated.  fill() blocks until `bytes` bytes are in
 * `dst` or the source ends; returns the bytes delivered. */
typedef struct { FILE *f; int sock; } source;

static size_t fill(source *src, uint8_t *dst, size_t bytes)
{
    if (src->f) return fread(dst, 1, bytes, src->f);
    size_t have = 0;
    while (have < bytes) {
        ssize_t n = recv(src->sock, dst + have, bytes - have, 0);   /* datagrams never straddle a request: see main() */
        if (n <= 0) break;                                           /* empty datagram = end of stream; error/timeout too */
        have += (size_t)n;
    }
    return have;
}

static void check(int rc, const char *what)
{
    if (rc < 0) { fprintf(stderr, "fm_replay: %s: %s\n", what, sdrhip_last_error()); exit(1); }
}

/* one stream over the bank (--stations: a row of audio blocks per station) or over the chain */
static int s16 = 0;   /* --s16: int16 IQ in, 4 bytes per sample */

static int make_stream(sdrhip_fm_stream **st, sdrhip_fm_chain *chain, sdrhip_fm_bank *bank, int bpp)
{
    if (s16) return sdrhip_fm_stream_create_bank_i16(st, bank, bpp * SOURCE_BLOCK, SOURCE_BLOCK);
    if (bank) return sdrhip_fm_stream_create_bank(st, bank, bpp * SOURCE_BLOCK, SOURCE_BLOCK);
    return sdrhip_fm_stream_create(st, chain, bpp * SOURCE_BLOCK, SOURCE_BLOCK);
}

/* the stream's pinned staging buffer and the push of what was written there, for either input type */
static uint8_t *input_buffer(sdrhip_fm_stream *st)
{
    return s16 ? (uint8_t *)sdrhip_fm_stream_input_buffer_i16(st) : sdrhip_fm_stream_input_buffer(st);
}

static int push(sdrhip_fm_stream *st, const uint8_t *buf, int n_samples)
{
    return s16 ? sdrhip_fm_stream_push_i16(st, (const int16_t *)buf, n_samples) : sdrhip_fm_stream_push(st, buf, n_samples);
}

/* the `ready` blocks of a de-emphasis Pipe, popped into `tmp` (SOURCE_BLOCK floats) and written to f */
static void drain(sdrhip_pipe *p, int ready, float *tmp, FILE *f)
{
    for (int i = 0; i < ready; i++) {
        int len = sdrhip_pipe_pop(p, tmp, SOURCE_BLOCK);
        check(len, "sdrhip_pipe_pop");
        fwrite(tmp, sizeof(float), (size_t)len, f);
    }
}

int main(int argc, char **argv)
{
    /* --shift NUM/DEN or --stations NUM/DEN[,...], anywhere on the line; what is left are the positional arguments */
    long long shift_num = 0, shift_den = 0;
    long long st_num[SDRHIP_FM_BANK_MAX_STATIONS], st_den[SDRHIP_FM_BANK_MAX_STATIONS];
    int stations = 0;
    double deemph_us = 0.0, audio_rate = 0.0;
    int have_deemph = 0, have_rate = 0;
    {
        int w = 1;
        for (int i = 1; i < argc; i++) {
            if (strcmp(argv[i], "--shift") == 0) {
                if (i + 1 >= argc || sscanf(argv[i + 1], "%lld/%lld", &shift_num, &shift_den) != 2 || shift_den < 1 || shift_den > 65536) {
                    fprintf(stderr, "fm_replay: --shift NUM/DEN with 1 <= DEN <= 65536\n");
                    return 2;
                }
                i++;
            } else if (strcmp(argv[i], "--deemph") == 0 || strcmp(argv[i], "--audio-rate") == 0) {
                const int is_tau = argv[i][2] == 'd';
                char *end = NULL;
                const double v = i + 1 < argc ? strtod(argv[i + 1], &end) : 0.0;
                if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(v > 0.0) || v > 1e12) {
                    fprintf(stderr, "fm_replay: --deemph TAU_US --audio-rate HZ, both positive\n");
                    return 2;
                }
                if (is_tau) { deemph_us = v; have_deemph = 1; } else { audio_rate = v; have_rate = 1; }
                i++;
            } else if (strcmp(argv[i], "--s16") == 0) {
                s16 = 1;
            } else if (strcmp(argv[i], "--stations") == 0) {
                const char *p = i + 1 < argc ? argv[i + 1] : "";
                int used = 0;
                while (stations < SDRHIP_FM_BANK_MAX_STATIONS && sscanf(p, "%lld/%lld%n", &st_num[stations], &st_den[stations], &used) == 2 &&
                       st_den[stations] >= 1 && st_den[stations] <= 65536) {
                    stations++;
                    p += used;
                    if (*p != ',') break;
                    p++;
                }
                if (stations < 1 || *p != '\0') {
                    fprintf(stderr, "fm_replay: --stations NUM/DEN[,NUM/DEN...] with 1 to %d stations, 1 <= DEN <= 65536\n", SDRHIP_FM_BANK_MAX_STATIONS);
                    return 2;
                }
                i++;
            } else {
                argv[w++] = argv[i];
            }
        }
        argc = w;
    }
    if (stations > 0 && shift_den > 0) { fprintf(stderr, "fm_replay: --shift or --stations, not both\n"); return 2; }
    if (have_deemph != have_rate) { fprintf(stderr, "fm_replay: --deemph TAU_US and --audio-rate HZ go together: both or neither\n"); return 2; }
    if (argc < 3) { fprintf(stderr, "usage: fm_replay [--s16] [--shift NUM/DEN | --stations NUM/DEN[,NUM/DEN...]] [--deemph TAU_US --audio-rate HZ] <iq_file | udp:PORT> <audio_f32_file> [blocks_per_push] [taps_prefix]\n"); return 2; }
    const int bpp = argc > 3 ? atoi(argv[3]) : 64;
    if (bpp < 1) { fprintf(stderr, "fm_replay: blocks_per_push must be >= 1\n"); return 2; }
    int n_decim, n_resamp, n_audio;
    const int is_udp = strncmp(argv[1], "udp:", 4) == 0;
    const char *prefix = argc > 4 ? argv[4] : argv[1];
    if (is_udp && argc <= 4) { fprintf(stderr, "fm_replay: udp source needs a taps_prefix\n"); return 2; }
    float *decim = read_floats(prefix, ".decim.f32", &n_decim);
    float *resamp = read_floats(prefix, ".resamp.f32", &n_resamp);
    float *audio_half = read_floats(prefix, ".audio_half.f32", &n_audio);

    sdrhip_fm_chain *chain = NULL;
    check(sdrhip_fm_chain_create(&chain, SDRHIP_ORDER_AVX, 8, decim, n_decim, 3, 10, resamp, n_resamp, audio_half, n_audio,
                                 0.2f, SOURCE_BLOCK), "sdrhip_fm_chain_create");
    if (shift_den > 0) {
        float *osc = (float *)malloc((size_t)shift_den * 2 * sizeof(float));
        check(sdrhip_tuner_shift_table(shift_num, shift_den, osc), "sdrhip_tuner_shift_table");
        check(sdrhip_fm_chain_set_tuner(chain, osc, (int)shift_den), "sdrhip_fm_chain_set_tuner");   /* copied */
        free(osc);
    }
    sdrhip_fm_bank *bank = NULL;
    const int per_station_files = stations > 0;
    const size_t sample_bytes = s16 ? 4 : 2;
    if (s16 && stations == 0) {
        /* int16 without --stations: a bank of one station, the --shift table or {1, 0} */
        stations = 1;
        st_num[0] = shift_den > 0 ? shift_num : 0;
        st_den[0] = shift_den > 0 ? shift_den : 1;
    }
    if (stations > 0) {
        float *tables[SDRHIP_FM_BANK_MAX_STATIONS];
        int periods[SDRHIP_FM_BANK_MAX_STATIONS];
        for (int j = 0; j < stations; j++) {
            tables[j] = (float *)malloc((size_t)st_den[j] * 2 * sizeof(float));
            periods[j] = (int)st_den[j];
            check(sdrhip_tuner_shift_table(st_num[j], st_den[j], tables[j]), "sdrhip_tuner_shift_table");
        }
        check(sdrhip_fm_bank_create(&bank, SDRHIP_ORDER_AVX, 8, decim, n_decim, 3, 10, resamp, n_resamp, audio_half, n_audio, 0.2f, SOURCE_BLOCK,
                                    stations, (const float *const *)tables, periods), "sdrhip_fm_bank_create");   /* copied */
        for (int j = 0; j < stations; j++) free(tables[j]);
    }
    sdrhip_fm_stream *st = NULL;
    check(make_stream(&st, chain, bank, bpp), "sdrhip_fm_stream_create");
    const int rows = sdrhip_fm_stream_rows(st);
    /* --deemph: one de-emphasis Pipe per row behind the stream; its blocks come out at the length they went in */
    sdrhip_pipe *de[SDRHIP_FM_BANK_MAX_STATIONS] = {NULL};
    if (have_deemph) {
        const float alpha = sdrhip_deemph_alpha(deemph_us * 1e-6, audio_rate);
        for (int j = 0; j < rows; j++) check(sdrhip_pipe_deemph(&de[j], alpha), "sdrhip_pipe_deemph");
        fprintf(stderr, "fm_replay: de-emphasis %g us at %g Hz: alpha = %.9g\n", deemph_us, audio_rate, (double)alpha);
    }

    source src = {NULL, -1};
    if (is_udp) {
        /* datagram sizes must divide the source block (the sender of tests/test_gpu_examples.py uses 4096 bytes), so a
         * recv() never has to split one */
        struct sockaddr_in addr;
        memset(&addr, 0, sizeof addr);
        addr.sin_family = AF_INET;
        addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
        addr.sin_port = htons((unsigned short)atoi(argv[1] + 4));
        src.sock = socket(AF_INET, SOCK_DGRAM, 0);
        int rcvbuf = 64 << 20;
        setsockopt(src.sock, SOL_SOCKET, SO_RCVBUF, &rcvbuf, sizeof rcvbuf);
        struct timeval tv = {20, 0};                                  /* a silent sender ends the stream */
        setsockopt(src.sock, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
        if (src.sock < 0 || bind(src.sock, (struct sockaddr *)&addr, sizeof addr) != 0) { perror("fm_replay: bind"); return 2; }
        {   /* warm the device up (module load, first allocations) on a throw-away stream, so that the first real push does
             * not stall long enough for the socket buffer to overflow */
            sdrhip_fm_stream *warm = NULL;
            check(make_stream(&warm, chain, bank, bpp), "sdrhip_fm_stream_create");
            uint8_t *wb = input_buffer(warm);
            if (!wb) check(-1, "sdrhip_fm_stream_input_buffer");
            memset(wb, s16 ? 0 : 128, (size_t)bpp * sample_bytes * SOURCE_BLOCK);
            for (int i = 0; i < 3; i++) check(push(warm, wb, bpp * SOURCE_BLOCK), "warm-up push");
            check(sdrhip_fm_stream_flush(warm), "warm-up flush");
            sdrhip_fm_stream_destroy(warm);
        }
        fprintf(stderr, "fm_replay: listening on 127.0.0.1:%d\n", atoi(argv[1] + 4));
        fflush(stderr);
    } else {
        src.f = fopen(argv[1], "rb");
    }
    /* one audio file per row: <audio_f32_file> itself, or with --stations <audio_f32_file>.<j> for station j */
    FILE *out[SDRHIP_FM_BANK_MAX_STATIONS];
    for (int j = 0; j < rows; j++) {
        char path[4096];
        if (per_station_files) snprintf(path, sizeof path, "%s.%d", argv[2], j);
        else snprintf(path, sizeof path, "%s", argv[2]);
        out[j] = fopen(path, "wb");
        if (!out[j]) { fprintf(stderr, "fm_replay: cannot open %s\n", path); return 2; }
    }
    if (!src.f && src.sock < 0) { fprintf(stderr, "fm_replay: cannot open input/output\n"); return 2; }
    float *block = (float *)malloc((size_t)rows * SOURCE_BLOCK * sizeof(float));
    float *deemphasised = (float *)malloc(SOURCE_BLOCK * sizeof(float));
    long long samples = 0, audio = 0;
    for (;;) {
        uint8_t *buf = input_buffer(st);   /* pinned: the upload needs no intermediate copy */
        if (!buf) check(-1, "sdrhip_fm_stream_input_buffer");
        size_t got = fill(&src, buf, (size_t)bpp * sample_bytes * SOURCE_BLOCK) / (sample_bytes * SOURCE_BLOCK);   /* whole source blocks only */
        int ready = 0;
        if (got > 0) {
            ready = push(st, buf, (int)got * SOURCE_BLOCK);
            check(ready, "sdrhip_fm_stream_push");
            samples += (long long)got * SOURCE_BLOCK;
        }
        if (got < (size_t)bpp) {
            ready = sdrhip_fm_stream_flush(st);
            check(ready, "sdrhip_fm_stream_flush");
        }
        for (int i = 0; i < ready; i++) {
            check(sdrhip_fm_stream_pop_rows(st, block, SOURCE_BLOCK, 1), "sdrhip_fm_stream_pop_rows");   /* one block of every row */
            for (int j = 0; j < rows; j++) {
                float *row = block + (size_t)j * SOURCE_BLOCK;
                if (!de[j]) { fwrite(row, sizeof(float), SOURCE_BLOCK, out[j]); continue; }
                int done = sdrhip_pipe_push(de[j], row, SOURCE_BLOCK);
                check(done, "sdrhip_pipe_push");
                drain(de[j], done, deemphasised, out[j]);
            }
            audio += SOURCE_BLOCK;
        }
        if (got < (size_t)bpp) break;
    }
    for (int j = 0; j < rows; j++) {
        if (!de[j]) continue;
        int done = sdrhip_pipe_flush(de[j]);
        check(done, "sdrhip_pipe_flush");
        drain(de[j], done, deemphasised, out[j]);
        sdrhip_pipe_destroy(de[j]);
    }
    if (per_station_files) fprintf(stderr, "fm_replay: %lld IQ samples in, %lld audio samples out for each of %d stations\n", samples, audio, rows);
    else fprintf(stderr, "fm_replay: %lld IQ samples in, %lld audio samples out\n", samples, audio);
    if (src.f) fclose(src.f);
    if (src.sock >= 0) close(src.sock);
    for (int j = 0; j < rows; j++) fclose(out[j]);
    free(block);
    free(deemphasised);
    sdrhip_fm_stream_destroy(st);
    sdrhip_fm_bank_destroy(bank);
    sdrhip_fm_chain_destroy(chain);
    free(decim);
    free(resamp);
    free(audio_half);
#ifdef SDRHIP_FAST_EXIT
    /* sanitizer builds only (examples/pipes_soak.c explains): skip the HIP runtime's static destructors */
    fflush(NULL);
    _exit(0);
#endif
    return 0;
}
