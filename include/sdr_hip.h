/*
 * sdr_hip.h -- C ABI of libsdr_hip.so: the MI355X (gfx950) implementation of the
 * streaming FIR / decimate / polyphase-resample / FM-demod / u8->cfloat hot path
 * of adamwalker/sdr.
 *
 * Three layers, all `extern "C"`, plain pointers and sizes only:
 *
 *  (1) DROP-IN SYMBOLS -- the reference's own native entry points, same names and
 *      signatures as c_sources/{convert,decimate,filter,resample,scale}.c, so the
 *      reference's `foreign import ccall unsafe "<sym>"` declarations
 *      (hs_sources/SDR/FilterInternal.hs:80-150,179-249,346-391; SDR/Util.hs:100-125)
 *      resolve against this library unchanged.  HOST pointers in, HOST pointers
 *      out, synchronous; results are bit-identical to the reference's x86 build
 *      (each variant keeps its own summation order).
 *
 *  (2) DEVICE STREAM API (sdrhip_*) -- descriptors that own prepared taps in HBM
 *      (the reference's Filter/Decimator/Resampler records, Filter.hs:116-144) and
 *      `_run` calls on DEVICE pointers, asynchronous on a caller-supplied HIP
 *      stream, addressed by GLOBAL stream index so that a contiguous sample
 *      stream can be cut into launches / shards anywhere without changing a bit.
 *
 *  (3) PIPE OPERATORS (sdrhip_pipe_*) -- the host-block push interface mirroring
 *      firFilter / firDecimator / firResampler / fmDemod /
 *      interleavedIQUnsignedByteToFloat (Filter.hs:532-727, Demod.hs:40-46,
 *      Util.hs:104-138): feed host blocks, receive host blocks of exactly
 *      blockSizeOut elements, pinned double-buffered hipMemcpyAsync inside.
 *
 * Stream semantics shared by (2) and (3).  Let a stage have interpolation I
 * (1 for filters/decimators), decimation D, and Pipe-visible length Lp
 * (numCoeffsF / numCoeffsD / numCoeffsR, i.e. the PADDED length).  Output m of
 * the whole stream has virtual window [m*D, m*D + Lp) in the I-times upsampled
 * input index space.  With `seam_block` = B > 0 (the size of the input blocks
 * the reference Pipe would have been fed), output m is
 *    "One"   (computed by the C SIMD kernel, lane order of `order`)  when its
 *            virtual window lies inside one input block, and
 *    "Cross" (computed by the pure-Haskell sequential kernel,
 *            FilterInternal.hs:397-423) when it straddles a multiple of B*I
 * -- exactly the split Filter.hs:536-727 makes, including its one irregular
 * case: when the first output that no longer fits a block already has its
 * first INPUT sample ceil(m*D/I) in the next block (only possible for I > 1
 * with filters shorter than the decimation step), the Pipe does not cross
 * over at that boundary (Filter.hs:707-709) and that output is the next
 * block's first "One".  seam_block = 0 means one
 * contiguous buffer: every output is "One" (what a single FFI call computes).
 *
 * Stream contract of layer (2) (tests/test_gpu_stream_order.py runs every family below behind a gate on a non-blocking stream).
 * ORDERED ON `stream`: every kernel, memset and copy a `_run` call makes on the caller's data -- the whole launch set: tile kernels
 * and their seam fix-up launches, the settle and repair launches of dcBlocker / agc, the mix + decimate pairs of the tuner's two-pass
 * route, hipFFT's transforms, the layers and finalise launches of a reduction -- is queued on `stream` in call order.  The call
 * reads d_in and workspaces, and writes d_out, d_final and states, only there: the caller may queue the producer of d_in before the
 * call and a consumer of d_out (or an overwrite of d_in) after it on the same stream, with no host synchronisation in between.
 * Scratch a descriptor owns and shares between calls (the tuner's leased lanes, the spectrum operator's work buffer) is handed from
 * one stream to the next with an event or a drain; a caller never orders it.
 * A FIRST RUN of a descriptor uploads its taps, tables, window and twiddles with blocking copies on the null stream (finished when
 * the call returns, before the first kernel it queues can start) and may allocate; it never waits for `stream`, but an allocation
 * may wait for the whole device.  The operators without a descriptor (convert, scale, fmDemod, amDemod, dcBlocker, agc and all
 * their row forms) have no first run.
 * MAY BLOCK THE HOST after the first run: (a) sdrhip_spectrum_run_device on the hipFFT route, and sdrhip_spectrum_reduce_run_device
 * on the hipFFT route or with a group of more than 32 rows, when `stream` is not the stream of the object's last such run: the call
 * waits on the host until that last stream has drained (one work buffer per object), and also when it needs a transform plan for a
 * batch size the object has not kept; (b) a tuner two-pass run (and so a tuner bank's or FM bank's channel-by-channel route through
 * it) whose chunk needs more scratch than its lane holds: it waits for the lane's last borrower and reallocates; (c) a run of a
 * shape that needs a larger internal buffer than any run before it.  Every other `_run` call -- the FIR stage operators and their
 * row forms, convert, scale, fmDemod, amDemod, dcBlocker, agc and their row forms, the tuner's fused route and its two-pass route at
 * a scratch size it has seen, the tuner bank, the FM chain without overlap mode, the FM bank, the spectrum operator's one-kernel
 * route with groups of at most 32 rows -- returns without having waited for `stream` or for any other stream.
 *
 * Errors: drop-in symbols cannot report (void returns): on a failure they call the
 * handler of sdrhip_set_error_handler and return, or -- without one -- print to stderr and abort().  sdrhip_* return SDRHIP_OK (0) or a negative code;
 * sdrhip_last_error() returns a thread-local message.
 */
#ifndef SDR_HIP_H
#define SDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* (1) Drop-in symbols.  Signatures are the reference's, verbatim.          */
/* ------------------------------------------------------------------------ */

/* c_sources/convert.c:15,22,37 -- num = number of BYTES (= floats out). */
void convertC(int num, uint8_t *in, float *out);
void convertCSSE(int num, uint8_t *in, float *out);
void convertCAVX(int num, uint8_t *in, float *out);
/* c_sources/convert.c:52,59,72 (BladeRF i16 -> f32) and :87 (f32 -> i16 TX) */
void convertCBladeRF(int num, int16_t *in, float *out);
void convertCSSEBladeRF(int num, int16_t *in, float *out);
void convertCAVXBladeRF(int num, int16_t *in, float *out);
void convertBladeRFTransmit(int num, float *in, int16_t *out);

/* c_sources/scale.c:15,22,30 */
void scale(int num, float factor, float *in_buf, float *out_buf);
void scaleSSE(int num, float factor, float *in_buf, float *out_buf);
void scaleAVX(int num, float factor, float *in_buf, float *out_buf);

/* c_sources/filter.c:16-68 -- real taps, real data.  num = outputs. */
void filterRR(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterSSERR(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterAVXRR(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
/* numCoeffs = HALF length (filter.c:50-68) */
void filterSSESymmetricRR(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterAVXSymmetricRR(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
/* c_sources/filter.c:73-147 -- real taps, complex data.  RC: SSE/AVX take
 * DUPLICATED taps (numCoeffs = 2P floats); RC2 / SymmetricRC take plain taps. */
void filterRC(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterSSERC(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterSSERC2(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterAVXRC(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterAVXRC2(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterSSESymmetricRC(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void filterAVXSymmetricRC(int num, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
/* c_sources/filter.c:152-161 */
void dcBlocker(int num, float lastSample, float lastOutput, float *finalSample, float *finalOutput,
               float *inBuf, float *outBuf);

/* c_sources/decimate.c:16-146 */
void decimateRR(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateSSERR(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateAVXRR(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateSSESymmetricRR(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateAVXSymmetricRR(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateRC(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateSSERC(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateSSERC2(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateAVXRC(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateAVXRC2(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateSSESymmetricRC(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);
void decimateAVXSymmetricRC(int num, int factor, int numCoeffs, float *coeffs, float *inBuf, float *outBuf);

/* c_sources/resample.c:16-142.  coeffs = table of num_groups HOST pointers to
 * zero-padded polyphase groups (FilterInternal.hs:335-342); returns end group.
 * Any number of polyphase groups, as in the reference (up to 64 the per-group offset tables travel as kernel arguments,
 * beyond that in device memory).  resampleRR needs decimation > interpolation and 0 <= filter_offset < interpolation
 * (outside these the reference's own recurrence leaves its arrays): then it prints the reason and abort()s -- it cannot
 * return an error.  The descriptor API (sdrhip_resampler_*) reports SDRHIP_ERR_ARG instead. */
void resampleRR(int buf_size, int coeff_size, int interpolation, int decimation, int filter_offset,
                float *coeffs, float *in_buf, float *out_buf);
int resample2RR(int buf_size, int num_coeffs, int starting_group, int num_groups, int *increments,
                float **coeffs, float *in_buf, float *out_buf);
int resampleSSERR(int buf_size, int num_coeffs, int starting_group, int num_groups, int *increments,
                  float **coeffs, float *in_buf, float *out_buf);
int resampleAVXRR(int buf_size, int num_coeffs, int starting_group, int num_groups, int *increments,
                  float **coeffs, float *in_buf, float *out_buf);
int resample2RC(int buf_size, int num_coeffs, int starting_group, int num_groups, int *increments,
                float **coeffs, float *in_buf, float *out_buf);
int resampleSSERC(int buf_size, int num_coeffs, int starting_group, int num_groups, int *increments,
                  float **coeffs, float *in_buf, float *out_buf);
int resampleAVXRC(int buf_size, int num_coeffs, int starting_group, int num_groups, int *increments,
                  float **coeffs, float *in_buf, float *out_buf);

/* NEW seam (the reference's fmDemod is pure Haskell, Demod.hs:21-46; SURVEY.md
 * 8(b) defines this FFI entry): out[i] = phase(in[i] * conj(in[i-1])), in[-1] =
 * (last_re,last_im).  HOST pointers. */
void fmDemodF(int num, float last_re, float last_im, const float *in_iq, float *out);

/* ------------------------------------------------------------------------ */
/* (2) Device stream API                                                    */
/* ------------------------------------------------------------------------ */

#define SDRHIP_OK            0
#define SDRHIP_ERR_ARG      (-1)  /* precondition violated (the reference's `assert` -> error) */
#define SDRHIP_ERR_HIP      (-2)  /* a HIP runtime call failed */
#define SDRHIP_ERR_NOMEM    (-3)
#define SDRHIP_ERR_STATE    (-4)

/* Summation order = which of the reference's variants is reproduced
 * (SDR.CPUID.featureSelect picks AVX on any host that has it, CPUID.hs:100-104). */
#define SDRHIP_ORDER_SCALAR  0    /* filterRR / decimateRC / resample2RR ...      */
#define SDRHIP_ORDER_SSE     1    /* 4 real / 2 complex lanes                     */
#define SDRHIP_ORDER_AVX     2    /* 8 real / 4 complex lanes                     */

const char *sdrhip_version(void);
const char *sdrhip_last_error(void);
/* Drop-in symbols return void, so a failure inside one (HIP error, out of memory, an argument the reference itself would
 * index out of bounds with) cannot be reported: by default they print the message and abort().  With a handler installed
 * (process-wide; NULL restores the default) the failing call instead records the message (sdrhip_last_error), calls
 * handler(code, message) and -- when the handler comes back -- returns to ITS caller at once, outputs unspecified.  A Haskell
 * host sets a flag in the handler and raises after the foreign call (haskell/SDR/GPU.hs: the reference raises from its
 * Pipes too, Filter.hs:526-527).  The handler must RETURN: it runs with C++ objects of the library live on the stack (a leased
 * scratch context among them), so a longjmp out of it is undefined behaviour and would strand that context. */
void sdrhip_set_error_handler(void (*handler)(int code, const char *message));
int sdrhip_device_count(void);
int sdrhip_set_device(int dev);
int sdrhip_device_name(char *buf, int buflen);
/* Tuning / test knob: the "short seamed launch" scale v.  A launch with seam_block > 0 that is short enough to be
 * launch-bound decides its One / Cross outputs inside ONE kernel instead of a tiled kernel plus a fix-up launch for the
 * seam outputs: real filters up to v/2 outputs and real resamplers up to 2v outputs take the generic kernel, the tiled
 * complex decimator computes its seam outputs in place up to 5v outputs.  Results are identical either way.
 * Default v = 32768 (also: environment SDRHIP_SMALL_LAUNCH); 0 = always the tiled kernels + fix-up launches; negative =
 * restore the default.  Returns the previous value. */
int sdrhip_set_small_launch_outputs(int outputs);

/* Thin memory / stream helpers so a non-C++ host (Haskell, ctypes) needs no HIP
 * bindings of its own.  `stream` arguments are hipStream_t passed as void*
 * (NULL = the default stream). */
int sdrhip_malloc(void **dptr, size_t bytes);
int sdrhip_free(void *dptr);
int sdrhip_malloc_host(void **hptr, size_t bytes);   /* pinned */
int sdrhip_free_host(void *hptr);
int sdrhip_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int sdrhip_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int sdrhip_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int sdrhip_stream_create(void **stream);
int sdrhip_stream_destroy(void *stream);
int sdrhip_stream_sync(void *stream);

/* Non-finite input to the FIR operators (filter, decimator, resampler: this descriptor API, the drop-in symbols and the Pipes):
 * an output is NaN exactly where the reference's x86 kernels give NaN -- also where a zero tap, the zero padding included, meets an
 * infinity -- but a NaN's sign and payload are unspecified (x86 generates 0xffc00000, this device 0x7fc00000, and which operand's
 * payload a sum keeps follows the order of evaluation).  Everything else is exact: +0 and -0, subnormal results (no flush to
 * zero), +Inf and -Inf, sums that overflow in the reference's own order.  u8 input on a descriptor with a nonzero tap below 2^-119
 * takes the generic kernel instead of the u8-fused ones (taps / 128 would not be exact): same results, fewer samples per second. */

/* ---- Filter (Filter.hs:116-120; constructors :163-261) ------------------- */
typedef struct sdrhip_filter sdrhip_filter;
/* fastFilter{C,SSE,AVX}{R,C}: zero-pads to the order's SIMD multiple
 * (mkFilter Filter.hs:167-175 / mkFilterC :196-209). data_complex: 0 real, 1 complex. */
int sdrhip_filter_create(sdrhip_filter **f, int order, int data_complex, const float *coeffs, int ncoeffs);
/* fastFilterSym{SSE,AVX}R (mkFilterSymR Filter.hs:234-245): half = first half of an
 * even-length linear-phase filter; nhalf must be a multiple of 4 (SSE) / 8 (AVX). */
int sdrhip_filter_sym_create(sdrhip_filter **f, int order, const float *half, int nhalf);
int sdrhip_filter_num_coeffs(const sdrhip_filter *f);            /* numCoeffsF */
void sdrhip_filter_destroy(sdrhip_filter *f);
/* out[k - k_begin] = stream output k, k in [k_begin,k_end); d_in[0] is stream input
 * element in_base (floats for real data, (re,im) pairs for complex).  The caller
 * guarantees d_in covers inputs [k_begin, k_end - 1 + numCoeffsF). */
int sdrhip_filter_run(const sdrhip_filter *f, void *stream, const float *d_in, int64_t in_base,
                      float *d_out, int64_t k_begin, int64_t k_end, int64_t seam_block);

/* ---- Decimator (Filter.hs:126-131; constructors :277-371) ---------------- */
typedef struct sdrhip_decimator sdrhip_decimator;
int sdrhip_decimator_create(sdrhip_decimator **d, int order, int data_complex, int factor,
                            const float *coeffs, int ncoeffs);
int sdrhip_decimator_sym_create(sdrhip_decimator **d, int order, int factor, const float *half, int nhalf);
int sdrhip_decimator_num_coeffs(const sdrhip_decimator *d);      /* numCoeffsD */
int sdrhip_decimator_factor(const sdrhip_decimator *d);
void sdrhip_decimator_destroy(sdrhip_decimator *d);
/* needs inputs [k_begin*factor, (k_end-1)*factor + numCoeffsD) */
int sdrhip_decimator_run(const sdrhip_decimator *d, void *stream, const float *d_in, int64_t in_base,
                         float *d_out, int64_t k_begin, int64_t k_end, int64_t seam_block);
/* same, reading interleaved u8 IQ (the u8->cfloat conversion of convert.c:37-50
 * fused into the loader; complex decimators only) */
int sdrhip_decimator_run_u8(const sdrhip_decimator *d, void *stream, const uint8_t *d_in_iq, int64_t in_base,
                            float *d_out, int64_t k_begin, int64_t k_end, int64_t seam_block);

/* ---- Tuner: a periodic complex oscillator mixed into the complex decimator -------- */
/* `P.map (VG.zipWith (*) osc) >-> firDecimator deci n` as ONE device operator: move a part of the band to 0 Hz, then low-pass and
 * decimate there (oscillators: quarterBandUp / halfBandUp, Util.hs:263-285; the product: Data.Complex's (*) at Float).  With n the
 * ABSOLUTE stream index of an input sample and N = period:
 *     x[n] = the input sample (u8 IQ: (u - 128) * (1/128) as convert.c; cfloat: as given)
 *     o[n] = osc[n mod N]
 *     m[n] = (x.re*o.re - x.im*o.im,  x.re*o.im + x.im*o.re)         f32, every product and every sum rounded, no FMA
 *     y[k] = what sdrhip_decimator_run computes on m                  same order, same One / Cross rule
 * The result equals, bit for bit, sdrhip_decimator_run applied to a buffer that already holds m, for every order, seam_block,
 * in_base and cut into launches.  The mix is computed in full for every entry (no shortcut for 0 or +-1: the sign of a zero
 * would change).  The oscillator phase depends on the absolute index alone, not on seam_block: N need not divide the block size.
 * Inputs and table must be finite (NaN payloads are out of contract).  The (*) parity is argued from GHC base's formula
 * (Data.Complex: (x:+y) * (x':+y') = (x*x'-y*y') :+ (x*y'+y*x')), no GHC ran.
 * The taps are prepared exactly as sdrhip_decimator_create(order, data_complex = 1, ...) prepares them; osc_iq = period (re, im)
 * float32 pairs, copied; period 1 .. 65536.  A descriptor is immutable after create (but for set_route) and may be shared by
 * host threads; it belongs to the device of its first run. */
typedef struct sdrhip_tuner sdrhip_tuner;
int sdrhip_tuner_create(sdrhip_tuner **t, int order, int factor, const float *coeffs, int ncoeffs, const float *osc_iq,
                        int period);
int sdrhip_tuner_num_coeffs(const sdrhip_tuner *t);              /* numCoeffsD */
int sdrhip_tuner_factor(const sdrhip_tuner *t);
int sdrhip_tuner_period(const sdrhip_tuner *t);
void sdrhip_tuner_destroy(sdrhip_tuner *t);
/* Ranges and guaranteed inputs as sdrhip_decimator_run: d_in[0] is stream sample in_base, the caller guarantees inputs
 * [k_begin*factor, (k_end-1)*factor + numCoeffsD); k_begin >= 0.  SDRHIP_ERR_ARG before any device work for a null handle or a
 * seam_block shorter than the filter.  Asynchronous on `stream`. */
int sdrhip_tuner_run(const sdrhip_tuner *t, void *stream, const float *d_in, int64_t in_base, float *d_out,
                     int64_t k_begin, int64_t k_end, int64_t seam_block);
int sdrhip_tuner_run_u8(const sdrhip_tuner *t, void *stream, const uint8_t *d_in_iq, int64_t in_base, float *d_out,
                        int64_t k_begin, int64_t k_end, int64_t seam_block);
/* 16-bit signed IQ (the BladeRF's samples): d_in_iq is interleaved (I, Q) int16, element i of the stream is d_in_iq[2 (i - in_base)]
 * and [... + 1], lengths and positions in complex samples as for u8.  With c(s) = (float)s * 2^-11 for EVERY int16 s (convertCBladeRF,
 * convert.c:52-85; exact in f32, c(0) = +0) the call writes, bit for bit, what sdrhip_tuner_run writes from the cfloat buffer
 * sdrhip_convert_i16_run makes of the same int16 buffer -- nothing new is argued.  The conversion happens first, in the kernels'
 * loaders (then the mix, then the taps; the 2^-11 is folded neither into the taps nor into the table: a product that underflows does
 * not commute with a power of two).  Routes as below: 1 = fused is the tuner bank's int16 tile kernel with one channel
 * (sdrhip_debug_tuner_i16_launches counts it, sdrhip_debug_tuner_fused_launches does not), its first window (d_in_iq + 4 bytes per
 * sample) 16-byte aligned; 2 = two-pass with an int16 mix kernel.  d_in_iq must be 4-byte aligned on every route (SDRHIP_ERR_ARG). */
int sdrhip_tuner_run_i16(const sdrhip_tuner *t, void *stream, const int16_t *d_in_iq, int64_t in_base, float *d_out,
                         int64_t k_begin, int64_t k_end, int64_t seam_block);
/* process-wide: launches of the int16 tile kernel, from a bank or from a one-row tuner (tests assert that no conversion pass stood in) */
long long sdrhip_debug_tuner_i16_launches(void);
/* Routes (same bits).  1 = fused: one tile kernel whose loader converts, fetches the oscillator entry and mixes on the way into
 * LDS, so m never reaches memory -- AVX order, factor 4 / 8 / 16, up to 128 prepared taps, seam_block >= 0, a 16-byte aligned
 * first window; a launch outside that returns SDRHIP_ERR_ARG.  2 = two-pass: a mix kernel writes m into a bounded
 * scratch buffer chunk by chunk and the stock decimator runs on it (every order and factor).  0 = auto (default): fused wherever
 * it applies, else two-pass. */
int sdrhip_tuner_set_route(sdrhip_tuner *t, int route);
long long sdrhip_debug_tuner_fused_launches(void);   /* process-wide: launches of the fused tile kernel (tests assert the route) */
/* test knob: samples one chunk of the two-pass route mixes at a time (<= 0: the default, 2^22); returns the previous value */
int64_t sdrhip_debug_set_tuner_chunk(int64_t samples);
/* osc[n] = exp(2 pi i ((num n) mod den) / den), n = 0 .. den - 1, as den (re, im) float32 pairs.  Pure host code, no device.
 * (1, 4) is quarterBandUp and (1, 2) is halfBandUp, bit for bit, zeros +0; a negative num shifts down.  1 <= den < 2^31.
 * The reduction, so that the table can be reproduced elsewhere (integers exact, `pi` = the double 3.141592653589793):
 *     r = (num n) mod den in [0, den);  q = floor(4 r / den) the quarter turn, f = 4 r - q den in [0, den)
 *     f = 0:        (c, s) = (1, 0)
 *     2 f = den:    c = s = (float)cos(pi * 0.25)                                  an odd eighth: |re| == |im|
 *     2 f < den:    phi = pi * ((double)f / (double)(2 den));        c = (float)cos(phi), s = (float)sin(phi)
 *     2 f > den:    phi = pi * ((double)(den - f) / (double)(2 den)); c = (float)sin(phi), s = (float)cos(phi)
 *     q = 0: (c, s);  q = 1: (0 - s, c);  q = 2: (0 - c, 0 - s);  q = 3: (s, 0 - c)     0 - x in float32: -x, and +0 for x = 0
 * cos / sin are the double-precision library functions of an angle in (0, pi/4), rounded once to float32. */
int sdrhip_tuner_shift_table(int64_t num, int64_t den, float *osc_iq /* den pairs */);

/* ---- Tuner bank: every channel of one capture as complex baseband rows ------------ */
/* K tuners of the same decimator, each with an oscillator table of its own, over ONE input.
 * Definition: channel j's row is d_out + j * out_stride floats; it holds outputs [k_begin, k_end) as (re, im) pairs and equals, bit
 * for bit, what sdrhip_tuner_run / sdrhip_tuner_run_u8 writes for the same (d_in, in_base, k_begin, k_end, seam_block) from a
 * sdrhip_tuner created with (order, factor, coeffs, ncoeffs, osc_iq[j], periods[j]) -- on every route of the bank, for every
 * seam_block, in_base, cut into launches and out_stride.  Nothing new is argued: the (*) parity and the One / Cross rule are the
 * tuner's.  Floats of d_out outside the K rows' [0, 2 (k_end - k_begin)) are not touched.
 * Create: tables and periods as sdrhip_fm_bank_create -- copied, period 1 .. 65536, every entry finite, 1 .. 32 channels; a channel
 * on the centre frequency takes the table {1, 0}.  SDRHIP_ERR_ARG (and *b = NULL) for whatever sdrhip_tuner_create refuses, a null
 * table pointer, a channel count outside 1 .. 32 and a non-finite table entry.
 * Run: SDRHIP_ERR_ARG before any device work, with nothing written, for whatever sdrhip_tuner_run refuses, out_stride <
 * 2 (k_end - k_begin) with more than one channel, an odd out_stride (rows stay 8-byte aligned) and route 1 forced on a launch the
 * banked kernel does not serve.  An empty range is SDRHIP_OK.  Asynchronous on `stream`; after the first run a run makes no
 * allocation, no host synchronisation and no host-to-device copy on the banked route (each channel's phase at the launch's first
 * sample and the row stride travel in the kernel's arguments).  A bank is immutable after create (but for set_route) and may be
 * shared by host threads; it belongs to the device of its first run. */
#define SDRHIP_TUNER_BANK_MAX_CHANNELS 32
typedef struct sdrhip_tuner_bank sdrhip_tuner_bank;
int sdrhip_tuner_bank_create(sdrhip_tuner_bank **b, int order, int factor, const float *coeffs, int ncoeffs, int channels,
                             const float *const *osc_iq, const int *periods);
void sdrhip_tuner_bank_destroy(sdrhip_tuner_bank *b);
int sdrhip_tuner_bank_channels(const sdrhip_tuner_bank *b);
int sdrhip_tuner_bank_period(const sdrhip_tuner_bank *b, int channel);
int sdrhip_tuner_bank_num_coeffs(const sdrhip_tuner_bank *b);    /* numCoeffsD */
int sdrhip_tuner_bank_factor(const sdrhip_tuner_bank *b);
int sdrhip_tuner_bank_run(const sdrhip_tuner_bank *b, void *stream, const float *d_in, int64_t in_base, float *d_out,
                          int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block);
int sdrhip_tuner_bank_run_u8(const sdrhip_tuner_bank *b, void *stream, const uint8_t *d_in_iq, int64_t in_base, float *d_out,
                             int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block);
/* 16-bit signed IQ, as sdrhip_tuner_run_i16: every row holds, bit for bit, what sdrhip_tuner_bank_run writes from the cfloat buffer
 * sdrhip_convert_i16_run makes of the same int16 buffer, on every route, for every seam_block, in_base, cut into launches and
 * out_stride.  Refusals as sdrhip_tuner_bank_run_u8, plus a d_in_iq that is not 4-byte aligned.  Routes: 1 = the banked launch of the
 * int16 tile kernel (it counts in sdrhip_debug_tuner_bank_launches AND in sdrhip_debug_tuner_i16_launches), 2 = sdrhip_tuner_run_i16
 * channel by channel, 0 = auto.  Auto rule for int16 input, with n = (k_end - k_begin) * factor:
 *     banked  iff  channels >= 2  and  n <= 2^24
 * read from `tools/tuner_bank_bench.py --i16` (profiles/tuner_i16_bench.txt: 1 / 2 / 4 / 8 / 12 / 32 channels x 8192, 2^17, 2^20 and 2^24
 * input samples, 128 taps / 8, 7 rounds) by the criterion of the rule below: at every measured point with K >= 2 the banked launch's
 * slowest round was below the K sdrhip_tuner_run_i16 calls' fastest, so the sweep confirms the u8 / cfloat rectangle and both bounds are
 * its edges; nothing beyond 2^24 samples per launch is measured.  One channel goes to its tuner, which for int16 is the same kernel with
 * one channel (measured level: 0.995 .. 1.001). */
int sdrhip_tuner_bank_run_i16(const sdrhip_tuner_bank *b, void *stream, const int16_t *d_in_iq, int64_t in_base, float *d_out,
                              int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block);
/* Routes (same bits).  1 = the banked launch: the tuner's fused tile kernel with a channel axis, one launch for all channels (and one
 * fix-up launch for all channels where the tuner's fused route takes one) -- the shapes of the tuner's route 1: AVX order, factor
 * 4 / 8 / 16, up to 128 prepared taps, seam_block >= 0, a 16-byte aligned first window; a launch outside that is SDRHIP_ERR_ARG.
 * 2 = channel by channel: sdrhip_tuner_run of the bank's own K tuners (their route auto) one after the other on the caller's stream.
 * 0 = auto (default): the banked launch where it fits AND the launch lies in the part of the measured rectangle where the banked
 * launch's slowest round was below the K tuner runs' fastest (tools/tuner_bank_bench.py, profiles/tuner_bank_bench.txt: 1 / 2 / 4 /
 * 8 / 12 / 32 channels x launches of 8192, 2^17, 2^20 and 2^24 input samples, 128 taps / 8, u8 and cfloat input, 7 rounds); everything
 * else, and everything outside that rectangle, goes channel by channel.  The rule, with n = (k_end - k_begin) * factor the input
 * samples of the launch:
 *     banked  iff  channels >= 2  and  n <= 2^24                                  (u8 and cfloat input alike)
 * Every measured point with K >= 2 is banked by that criterion, so both bounds are edges of the rectangle, not crossovers.  One channel
 * is one launch either way and was NOT level for cfloat input (8.1 against 7.6 us at 8192 samples, 37.0 against 35.1 at 2^24): it goes
 * to its tuner.  Launches of the other factors and of fewer taps, and launches shorter than 8192 samples, are held to the same bound
 * in input samples (no more arithmetic per sample, no less launch-bound); nothing beyond 2^24 samples per launch is measured. */
int sdrhip_tuner_bank_set_route(sdrhip_tuner_bank *b, int route);   /* 0 auto, 1 banked launch, 2 channel by channel */
long long sdrhip_debug_tuner_bank_launches(void);                   /* banked launches, process-wide */
/* launches of the all-Cross kernel of the bank's Pipe (sdrhip_pipe_tuner_bank: the boundary part of a ragged push), process-wide;
 * sdrhip_tuner_bank_run never takes it */
long long sdrhip_debug_tuner_bank_cross_launches(void);

/* ---- Resampler (Filter.hs:137-144; constructors :408-502) ---------------- */
typedef struct sdrhip_resampler sdrhip_resampler;
int sdrhip_resampler_create(sdrhip_resampler **r, int order, int data_complex, int interpolation,
                            int decimation, const float *coeffs, int ncoeffs);
int sdrhip_resampler_num_coeffs(const sdrhip_resampler *r);      /* numCoeffsR */
int sdrhip_resampler_num_groups(const sdrhip_resampler *r);
void sdrhip_resampler_destroy(sdrhip_resampler *r);
/* Closed form of the phase recurrence (Filter.hs:613-641): first input element and
 * filter offset of stream output m (stream starting at phase 0). */
int64_t sdrhip_resampler_in_offset(const sdrhip_resampler *r, int64_t m);
int sdrhip_resampler_filter_offset(const sdrhip_resampler *r, int64_t m);
int sdrhip_resampler_group(const sdrhip_resampler *r, int64_t m);
/* out_block: the output block size of the Pipe being reproduced (firResampler's blockSizeOut; 0 =
 * unbounded).  It matters for one output in ~10^4 seams: inside a crossover the reference computes
 * the output whose virtual start lies in the last I-1 zero-stuffed positions before the boundary
 * sequentially, unless its output block was full just before it (Filter.hs:715,722-724).
 * Needs inputs [in_offset(k_begin), in_offset(k_end - 1) + numCoeffsR / interpolation). */
int sdrhip_resampler_run(const sdrhip_resampler *r, void *stream, const float *d_in, int64_t in_base,
                         float *d_out, int64_t k_begin, int64_t k_end, int64_t seam_block,
                         int64_t out_block);

/* ---- element-wise stages -------------------------------------------------- */
/* interleavedIQUnsignedByteToFloat (Util.hs:104-138 / convert.c): n_bytes u8 -> n_bytes f32 */
int sdrhip_convert_u8_run(void *stream, const uint8_t *d_in, float *d_out, int64_t n_bytes);
int sdrhip_convert_i16_run(void *stream, const int16_t *d_in, float *d_out, int64_t n);
int sdrhip_scale_run(void *stream, float factor, const float *d_in, float *d_out, int64_t n);
/* fmDemod (Demod.hs:40-46).  y[k] for k in [k_begin,k_end); the sample preceding
 * k_begin is d_in[k_begin-1-in_base] when k_begin > in_base, else (last_re,last_im)
 * (the Pipe's carried state; (0,0) at stream start, Demod.hs:41). */
int sdrhip_fm_demod_run(void *stream, const float *d_in_iq, int64_t in_base, float *d_out,
                        int64_t k_begin, int64_t k_end, float last_re, float last_im);
/* amDemod: the AM receiver's envelope detector, `P.map (VG.map magnitude)`.  n interleaved complex float32 samples ->
 * n float32, d_out[i] = magnitude(d_in_iq[2i], d_in_iq[2i+1]) with GHC base's Data.Complex.magnitude at Float, the
 * function sdrhip_agc_run steps with.  Every step f32, no FMA:
 *     k = max(exponent re, exponent im)                      -- exponent 0 = 0, else frexp's (denormals normalised)
 *     m = ldexpf(sqrtf(a*a + b*b), k),  a = ldexpf(re, -k), b = ldexpf(im, -k)          -- correctly rounded sqrt
 * which is neither sqrtf(re*re + im*im) nor hypotf.  The definition's consequences are the reference's and are kept:
 * magnitude(1e-30, 0) = +0 (k = 0, the square underflows), magnitude(1e-30, 1e-30) = 0x0de57822, magnitude(FLT_MAX, 1)
 * = FLT_MAX.  Non-finite input is in contract: a NaN part gives NaN (payload unspecified), otherwise an infinite part
 * gives +Inf.  The parity with `base` is argued, not executed, as for agc.
 * Asynchronous on `stream`; exactly one kernel launch for any n > 0; n == 0 is SDRHIP_OK with no launch.  Any
 * 4-byte-aligned pointers: 16-byte loads and stores where d_in_iq, respectively d_out, is 16-byte aligned, else 8- or
 * 4-byte ones, the two sides chosen independently.  No float outside [0, 2n) of d_in_iq is read, none outside [0, n) of
 * d_out written.  Not in-place.  SDRHIP_ERR_ARG, before any device work and with nothing written: a null pointer, n < 0,
 * d_in_iq == d_out. */
int sdrhip_am_demod_run(void *stream, const float *d_in_iq, float *d_out, int64_t n);
/* Diagnostics: kernel launches of sdrhip_am_demod_run and sdrhip_am_demod_run_rows, process-wide. */
long long sdrhip_debug_am_demod_launches(void);
/* Diagnostics: how many stream-API launches the general LDS-tiled kernels (kernels_split.hip) have served in
 * this process -- the tests use it to prove the tiled path, not the one-thread-per-output fallback, ran. */
long long sdrhip_debug_tiled_launches(void);

/* dcBlocker (c_sources/filter.c:152-161; Pipe dcBlockingFilter, Filter.hs:730-739) on device memory:
 * y[i] = (float)((double)(x[i] - x[i-1]) + 0.997 * (double)y[i-1]), x[-1] = last_sample, y[-1] = last_output.
 * Bit-identical to the sequential loop (speculative chunks, verified and settled on the device).
 * d_final receives {finalSample, finalOutput}; n == 0 writes {last_sample, last_output} there.  d_workspace
 * may be NULL (sequential walk); when given it starts with three uint32 statistics {chunks left to the
 * sequential settle pass, samples it rewrote, chunks recomputed by the parallel repair rounds} -- all zero when
 * every speculation converged -- and a fourth word, the chunks the launch speculated on (0 = sequential walk).
 * run_in = samples each chunk runs in before its first output, rounded up to a multiple of 4 (0 = default 12288;
 * a shorter run-in does less redundant work but leaves more chunks to settle; the result never depends on it);
 * blocks shorter than two run-ins take the sequential walk, whatever run_in is.  Not in-place. */
size_t sdrhip_dc_blocker_workspace_bytes(int64_t n);
int sdrhip_dc_blocker_run(void *stream, const float *d_in, float *d_out, int64_t n, float last_sample,
                          float last_output, float *d_final, void *d_workspace, size_t workspace_bytes,
                          int run_in);
/* Diagnostics: the plan sdrhip_dc_blocker_run follows for these arguments when it has a workspace.  Returns the number
 * of chunks (0 = sequential walk); *chunk and *run_in_used (either may be NULL) receive the chunk length and the run-in. */
int sdrhip_debug_dc_plan(int64_t n, int run_in, int64_t *chunk, int64_t *run_in_used);

/* agc (hs_sources/SDR/Util.hs:325-342; Pipe agcPipe, Util.hs:344-348) on device memory, interleaved complex samples.
 * Per sample (re, im), everything in f32, no FMA:
 *     c_re = re * state;  c_im = im * state                  -- the output sample
 *     m    = magnitude(c_re, c_im)
 *     state' = state + mu * (reference - m)
 * with GHC base's Data.Complex.magnitude at Float:
 *     k = max(exponent c_re, exponent c_im)                  -- exponent 0 = 0, else frexp's (denormals normalised)
 *     m = ldexpf(sqrtf(a*a + b*b), k),  a = ldexpf(c_re, -k), b = ldexpf(c_im, -k)      -- correctly rounded sqrt
 * which is not sqrtf(re*re + im*im): the two differ where a square under- or overflows.  Bit-identical to the
 * sequential loop for finite inputs whose trajectory stays finite (once the state is NaN its payload is unspecified).
 * d_final receives the final state (one float); n == 0 writes `state` there.  d_workspace may be NULL (sequential
 * walk); when given it starts with the three uint32 statistics of sdrhip_dc_blocker_run and a fourth word, the chunks
 * the launch speculated on (0 = sequential walk).  run_in = samples each chunk runs in before its first output
 * (0 = default, about 128 / mu: the contraction rate is mu * |x|); blocks shorter than two run-ins take the
 * sequential walk.  The result never depends on run_in.  Not in-place. */
size_t sdrhip_agc_workspace_bytes(int64_t n);       /* enough for any run_in */
int sdrhip_agc_run(void *stream, const float *d_in_iq, float *d_out_iq, int64_t n /* complex samples */,
                   float mu, float reference, float state, float *d_final /* 1 float: final state */,
                   void *d_workspace, size_t workspace_bytes, int run_in);
/* Diagnostics: the plan sdrhip_agc_run follows for these arguments when it has a workspace.  Returns the number of
 * chunks (0 = sequential walk); *chunk and *run_in_used (either may be NULL) receive the chunk length and the run-in. */
int sdrhip_debug_agc_plan(int64_t n, float mu, int run_in, int64_t *chunk, int64_t *run_in_used);

/* ---- row forms: every row of a bank (sdrhip_tuner_bank_run, sdrhip_fm_bank_run) in one launch set ----
 * Row r is d_in + r * in_stride -> d_out + r * out_stride, strides in floats.  Row r's output and final state are, bit
 * for bit, what the one-row call writes for that row alone from state d_state[r] (dcBlocker: the pair d_state[2r],
 * d_state[2r+1]), for any rows, strides, run_in, workspace or none, and whatever the other rows hold; the magnitude
 * parity and the NaN caveat are those of sdrhip_agc_run.  Floats of d_out outside the rows' [0, 2n) (dcBlocker and
 * fmDemod: [0, n)) are not touched.
 * States are device memory on both sides, so a stream of pushes needs no host synchronisation.  d_final may be the same
 * pointer as d_state: every read of d_state is ordered before the first write of d_final (a lane reads its row's state
 * before it writes it, or the reads are in a launch before the one that writes).  n == 0 copies the states and touches
 * nothing else.
 * d_workspace, when given, starts with rows x four uint32 statistics, row r's at word 4r, with the meanings of the
 * one-row operators.  NULL sends every row to the sequential walk: still one launch for all rows.
 * The plan is the one-row plan of (n, mu, run_in); the chunk grows, rounded up to 8 samples, only where rows x chunks
 * would pass the one-row lane cap (32768), so the route edge n == 2 * run-in does not depend on rows.
 * SDRHIP_ERR_ARG, before any device work and with nothing written: rows outside 1 .. SDRHIP_ROWS_MAX, a null pointer
 * (other than d_workspace), n < 0, run_in < 0, with rows > 1 a stride shorter than a row, an odd stride on an
 * interleaved-complex side (both of agc), d_in == d_out, a workspace smaller than *_rows_workspace_bytes(rows, n). */
#define SDRHIP_ROWS_MAX 1024
size_t sdrhip_agc_rows_workspace_bytes(int rows, int64_t n);
int sdrhip_agc_run_rows(void *stream, const float *d_in_iq, int64_t in_stride, float *d_out_iq, int64_t out_stride,
                        int rows, int64_t n /* complex samples per row */, float mu, float reference,
                        const float *d_state /* rows floats, device */, float *d_final /* rows floats, device */,
                        void *d_workspace, size_t workspace_bytes, int run_in);
/* As sdrhip_debug_agc_plan; rows == 1 gives exactly that plan. */
int sdrhip_debug_agc_rows_plan(int rows, int64_t n, float mu, int run_in, int64_t *chunk, int64_t *run_in_used);

size_t sdrhip_dc_blocker_rows_workspace_bytes(int rows, int64_t n);
int sdrhip_dc_blocker_run_rows(void *stream, const float *d_in, int64_t in_stride, float *d_out, int64_t out_stride,
                               int rows, int64_t n, const float *d_state /* rows x {last_sample, last_output} */,
                               float *d_final /* rows x {finalSample, finalOutput} */,
                               void *d_workspace, size_t workspace_bytes, int run_in);
int sdrhip_debug_dc_rows_plan(int rows, int64_t n, int run_in, int64_t *chunk, int64_t *run_in_used);

/* fmDemod over rows: in_base / k_begin / k_end as sdrhip_fm_demod_run, the same for every row.  Row r's predecessor of
 * k_begin is d_in[k_begin - 1 - in_base] of its row when k_begin > in_base, otherwise d_last_iq[2r], d_last_iq[2r+1].
 * d_last_out, if given, receives each row's sample k_end - 1; with an empty range the row's d_last_iq, or (0, 0) when
 * d_last_iq is NULL.  It is the next call's d_last_iq, and the two may be the same pointer (each row's pair is read
 * before it is written, by the same lane).  in_stride must be even, and with rows > 1 cover 2 * (k_end - in_base)
 * floats; out_stride k_end - k_begin. */
int sdrhip_fm_demod_run_rows(void *stream, const float *d_in_iq, int64_t in_stride, int64_t in_base, float *d_out,
                             int64_t out_stride, int rows, int64_t k_begin, int64_t k_end,
                             const float *d_last_iq /* rows x (re, im); NULL = (0, 0) */,
                             float *d_last_out /* NULL, or rows x (re, im) */);

/* Diagnostics: kernel launches of the row forms, process-wide: 1 per call on the sequential walk and for fmDemod, 5 per
 * call (speculate, three repair rounds, settle) with chunks. */
long long sdrhip_debug_rows_launches(void);

/* ---- de-emphasis: the one-pole low-pass behind an FM receiver's audio, one row or every row of a bank ----
 *     y[i] = y[i-1] + alpha * (x[i] - y[i-1])        y[-1] = state
 * Three f32 operations per sample, each rounded to nearest, in this order: subtract, multiply, add; no FMA.  The final state is
 * y[n-1], with n == 0 the state.  The reference has no de-emphasis: the definition is this library's, written as the reference
 * writes agc (a mapAccum at Float), and tests/deemph_model.py is its model.  Bit-identical to the sequential loop, final states
 * included, on every input whose trajectory stays finite; where the sequential loop holds a NaN the device holds a NaN, payload and
 * sign unspecified (an Inf sample, or an x - y that overflows, turns the state into NaN one or two steps later).
 * sdrhip_deemph_alpha is host arithmetic: (float)(1.0 - exp(-1.0 / (tau_seconds * sample_rate))) computed in double; 0.0f, a value the
 * run calls refuse, when either argument is not finite and positive.  75e-6 s at 48 kHz gives 0.2425..., at 256 kHz 0.0507....
 * Contract: that of the dcBlocker row form above.  Everything is ordered on `stream`, no host synchronisation; not in-place; states
 * are device arrays of `rows` floats on both sides and d_final may be d_state; n == 0 copies the states and touches nothing else;
 * floats outside the rows' [0, n) are untouched; rows 1 .. SDRHIP_ROWS_MAX; run_in = 0 is the default, ceil(40 / alpha) (about 1.5
 * times the slowest meeting of two trajectories seen, tests/test_deemph_model.py), any other value is rounded up to a multiple of 4,
 * and the result never depends on it.  sdrhip_deemph_run is the rows call with one row and `state` by value.
 * Routes (the auto rule).  1 SEQ: one workgroup per row, one lane walks the row; n < 2 * run-in, and n > 65536 without a workspace.  2 WG: ONE launch,
 * one workgroup per row, lane j owns chunk j (max(16, n / 1024 rounded up to 4) samples, at most 1024 chunks): it runs in, writes its
 * chunk, and the workgroup repeats rounds in which every chunk whose start state differs from its predecessor's end state is
 * recomputed, until a round finds no difference (at most `chunks` rounds); it fits 2 * run-in <= n <= 65536 and needs no workspace; auto
 * takes it there, except with a workspace from n = 32768 on.  3 LS: the dcBlocker rows launch set (speculate, three repair rounds,
 * settle; 5 launches), with a workspace, for n >= 32768 (and >= 2 * run-in).  The edge at 32768 is read from the sweep
 * (profiles/deemph_bench.txt: WG ahead of LS at 16384, LS ahead at 32768 and 65536, at 1 and 32 rows); the lower edge and the bound of
 * 65536 are the starting values, which the sweep could not move (README.md "And for de-emphasis").  An exactly constant row (silence, padding) does not let
 * trajectories meet; it is repaired chunk by chunk, up to the time of a sequential walk.
 * The access width is one for all rows: 16 / 8 / 4 bytes as the base pointers and, with rows > 1, the strides * 4 allow.
 * d_workspace is needed by LS only (*_workspace_bytes; NULL is fine on SEQ and WG).  When given it starts with rows x four uint32
 * statistics on every route.  SEQ: zeros.  LS: the dcBlocker's words.  WG: {rounds that recomputed a chunk, 0, chunks whose start
 * state was replaced summed over the rounds, chunks}.
 * SDRHIP_ERR_ARG, before any device work and with nothing written: alpha outside (0, 1] or not finite, rows out of range, a null
 * pointer other than d_workspace, n < 0, run_in < 0, d_in == d_out, with rows > 1 a stride shorter than n, a workspace smaller than
 * *_workspace_bytes, and a forced route (below) that does not fit. */
float sdrhip_deemph_alpha(double tau_seconds, double sample_rate);
size_t sdrhip_deemph_workspace_bytes(int64_t n);
int sdrhip_deemph_run(void *stream, const float *d_in, float *d_out, int64_t n, float alpha, float state,
                      float *d_final /* 1 float, device */, void *d_workspace, size_t workspace_bytes, int run_in);
size_t sdrhip_deemph_rows_workspace_bytes(int rows, int64_t n);
int sdrhip_deemph_run_rows(void *stream, const float *d_in, int64_t in_stride, float *d_out, int64_t out_stride,
                           int rows, int64_t n, float alpha, const float *d_state /* rows floats, device */,
                           float *d_final /* rows floats, device */, void *d_workspace, size_t workspace_bytes, int run_in);
/* Diagnostics.  The plan the run calls follow for these arguments and the route in force: returns the chunks per row (0 = SEQ),
 * *route (1 SEQ, 2 WG, 3 LS), *chunk and *run_in_used (each may be NULL); SDRHIP_ERR_ARG where the run call would refuse. */
int sdrhip_debug_deemph_plan(int rows, int64_t n, float alpha, int run_in, int has_workspace,
                             int *route, int64_t *chunk, int64_t *run_in_used);
/* 0 auto (the default), 1 SEQ, 2 WG, 3 LS, process-wide, for tests and tools: a forced route that does not fit a call (WG past its
 * bound, LS without a workspace, either below two run-ins) makes that call SDRHIP_ERR_ARG.  Pipes always follow the auto rule. */
void sdrhip_debug_set_deemph_route(int route);
/* kernel launches of the de-emphasis calls, process-wide: 1 per SEQ or WG call, 5 (one launch set) per LS call */
long long sdrhip_debug_deemph_launches(void);

/* ---- squelch: a gate decision per block from the block's mean power, one row or every row of a bank ----
 * A detector row (real, or complex when det_complex = 1; it may be the signal row itself) is cut into n_blocks blocks of block_det
 * samples, the signal row into as many blocks of block_sig floats.  The reference has no squelch: the definition is this library's,
 * and tests/squelch_model.py is its model.  Every operation is f32 and rounded, no FMA.
 * Power of a sample: x * x; complex: a = re * re, b = im * im, a + b.  Level of a block: 256 slots, slot[j] = the sum of the block's
 * powers p_i with i mod 256 == j in ascending i (an empty slot is +0); fold slot[j] += slot[j + w] (j < w) for w = 128, 64 .. 1;
 * level = slot[0] * (float)(1.0 / block_det).
 * Gate, block after block of a row, state {det, hang_left} (int32; a fresh stream starts from {0, 0}; on entry det is read as
 * det != 0 and hang_left is clamped into 0 .. hang_blocks):
 *     open_above = 1: want_open = level >= open_level, want_close = level <  close_level      (close_level <= open_level)
 *     open_above = 0: want_open = level <= open_level, want_close = level >  close_level      (close_level >= open_level)
 *     if want_open: det = 1; else if want_close: det = 0;            (a NaN level, or one between the two levels: det stays)
 *     if det: hang_left = hang_blocks, gate = 1; else if hang_left > 0: hang_left -= 1, gate = 1; else gate = 0
 * Output: with gate 1 the block's block_sig signal floats are copied bit for bit (NaN payloads included), with gate 0 they are +0.0f.
 * d_levels / d_gates, when given, receive every block's level and gate (rows x n_blocks, rows contiguous).  Consecutive calls over
 * consecutive whole blocks that hand d_final on as d_state are one stream and give the bits of one call.
 * Contract.  Everything is ordered on `stream`, no host synchronisation.  Row r is read and written at d_det + r * det_stride,
 * d_in + r * in_stride, d_out + r * out_stride (strides in floats); floats outside the rows' [0, n_blocks * block_sig) are untouched.
 * d_in == NULL && d_out == NULL is detect-only: state, levels and gates are written, block_sig is ignored.  n_blocks == 0 copies the
 * states (read as above) and touches nothing else.  d_det == d_in is self-detection.  d_out == d_in gates in place and needs
 * out_stride == in_stride; the levels are those of the samples as they were before the call.  d_out == d_det is allowed only when
 * d_det == d_in as well, and then the detector is real with block_det == block_sig and det_stride == in_stride (the rows coincide
 * block for block).  d_state NULL = {0, 0} for every row; d_final may be NULL, and may be d_state.  sdrhip_squelch_run is the rows
 * call with one row and the state by value.
 * Access width: 16 / 8 / 4 bytes, chosen on its own for the detector (from d_det, with rows > 1 det_stride, and with n_blocks > 1
 * the floats of a block), the signal and the output (from the pointer and, with rows > 1, the stride).
 * Routes.  1 WG: ONE launch, one workgroup of 16 waves per row, no workspace: one wave per block takes the levels (lane l holds
 * slots 4l .. 4l + 3), the workgroup finds the gates of up to 1024 blocks by two max-scans in LDS, copies the signal and writes the
 * state; a row of more than 1024 blocks is walked in groups of 1024 inside the workgroup.  2 LS: three launches (two when
 * detect-only): levels over blocks x rows, gate with one workgroup per row, apply over signal tiles x rows; it needs a workspace
 * (levels and gates: rows * n_blocks * 5 bytes + 64).  Auto rule: WG while n_blocks <= 1024 and a row's detector plus signal bytes
 * are <= 256 KiB; past either, LS when a workspace is given, WG when not.  Both edges are the starting values: README.md "And for
 * squelch" says what profiles/squelch_bench.txt could and could not tell about them.
 * SDRHIP_ERR_ARG, before any device work and with nothing written: rows outside 1 .. SDRHIP_ROWS_MAX; block_det or block_sig outside
 * 1 .. 2^20; n_blocks < 0 or a row of more than 2^40 floats; a level that is not finite or is negative; the levels in the wrong
 * order for the polarity; hang_blocks outside 0 .. 2^30; open_above or det_complex other than 0 / 1; a null d_det; one of d_in /
 * d_out null without the other; an odd det_stride with a complex detector; with rows > 1 a stride shorter than the row; the
 * aliasings not allowed above; a workspace smaller than *_workspace_bytes; a forced route (below) that does not fit. */
size_t sdrhip_squelch_rows_workspace_bytes(int rows, int64_t n_blocks);
int sdrhip_squelch_run_rows(void *stream, const float *d_det, int64_t det_stride, int det_complex, int block_det,
                            const float *d_in, int64_t in_stride, float *d_out, int64_t out_stride, int block_sig,
                            int rows, int64_t n_blocks, float open_level, float close_level, int hang_blocks, int open_above,
                            const int32_t *d_state /* rows x {det, hang_left}; NULL = {0, 0} */,
                            int32_t *d_final /* NULL, or rows x 2; may be d_state */,
                            float *d_levels /* NULL, or rows x n_blocks */, uint8_t *d_gates /* NULL, or rows x n_blocks */,
                            void *d_workspace, size_t workspace_bytes);
int sdrhip_squelch_run(void *stream, const float *d_det, int det_complex, int block_det, const float *d_in, float *d_out,
                       int block_sig, int64_t n_blocks, float open_level, float close_level, int hang_blocks, int open_above,
                       int32_t det, int32_t hang_left, int32_t *d_final /* NULL, or 2 int32 on the device */,
                       float *d_levels, uint8_t *d_gates, void *d_workspace, size_t workspace_bytes);
/* Diagnostics.  The route the run calls take for these arguments and the route in force (block_sig = 0: detect-only): returns the
 * kernel launches of such a call (1 on WG; 3 on LS, 2 when detect-only) and *route (1 WG, 2 LS; may be NULL); SDRHIP_ERR_ARG where
 * the run call would refuse the sizes or the route. */
int sdrhip_debug_squelch_plan(int rows, int64_t n_blocks, int block_det, int det_complex, int block_sig, int has_workspace,
                              int *route);
/* 0 auto (the default), 1 WG, 2 LS, process-wide, for tests and tools: forced LS without a workspace makes a call SDRHIP_ERR_ARG
 * (n_blocks == 0 is always the one state-copying launch). */
void sdrhip_debug_set_squelch_route(int route);
/* kernel launches of the squelch calls, process-wide */
long long sdrhip_debug_squelch_launches(void);

/* amDemod over rows: row r's n samples at d_in_iq + r * in_stride -> n floats at d_out + r * out_stride, bit for bit the
 * one-row call (sdrhip_am_demod_run) on that row, whatever the other rows hold; it is the same kernel with the row on
 * the grid's second axis.  Exactly one launch for any rows and n > 0 (the workgroups loop over a row's samples, so no
 * grid limit cuts a call); none for n == 0.  The access width is one for all rows: 16 / 8 / 4-byte loads as d_in_iq and
 * in_stride * 4 allow, 16 / 8 / 4-byte stores as d_out and out_stride * 4 allow.  Floats of d_out outside the rows'
 * [0, n), and of d_in_iq outside their [0, 2n), are not touched.  Launches count in sdrhip_debug_am_demod_launches, not
 * in sdrhip_debug_rows_launches.
 * SDRHIP_ERR_ARG, before any device work and with nothing written: rows outside 1 .. SDRHIP_ROWS_MAX, a null pointer,
 * n < 0, d_in_iq == d_out, and with rows > 1 in_stride < 2n, an odd in_stride, out_stride < n. */
int sdrhip_am_demod_run_rows(void *stream, const float *d_in_iq, int64_t in_stride, float *d_out, int64_t out_stride,
                             int rows, int64_t n);

/* ---- AM receiver bank: every channel's envelope (and dcBlocker) from one capture ---- */
/* The AM receiver of the reference's Readme (tuner, decimator, `magnitude`, dcBlocker) for the K channels of a tuner bank.
 * Definition: channel j's row is d_out + j * out_stride floats and holds k_end - k_begin floats; they equal, bit for bit, what
 * sdrhip_tuner_bank_run / _run_u8 / _run_i16 writes into complex rows for the same (d_in, in_base, k_begin, k_end, seam_block), put
 * through sdrhip_am_demod_run_rows and then, with dc_block = 1, through sdrhip_dc_blocker_run_rows from the state d_dc_state, with a
 * workspace and the default run-in, its final state written back to d_dc_state -- on every route, for every seam_block, in_base, cut
 * into launches and out_stride.  Nothing new is argued: the (*) parity and the One / Cross rule are the tuner's, `magnitude` is
 * amDemod's, dcBlocker is dcBlocker.  Floats of d_out outside the K rows' [0, k_end - k_begin) are not touched.
 * d_dc_state: 2 K device floats, channel j's (lastSample, lastOutput) at [2j, 2j + 2), read and written; NULL if and only if
 * dc_block = 0.  THE STATE BELONGS TO OUTPUT k_begin: it is dcBlocker's state in front of that output, and after the run it is the
 * state in front of output k_end.  Consecutive runs over consecutive ranges [k0, k1), [k1, k2), ... that reuse one state array, on one
 * stream, are ONE stream and give the bits of one run over [k0, kn); a stream starts from zeros (`func 0 0`, Filter.hs:731).  Two
 * streams (two host threads on one bank) take two state arrays and two workspaces.
 * Create: the tuner bank is BORROWED and must outlive the AM bank; SDRHIP_ERR_ARG (and *b = NULL) for a null bank and a dc_block
 * outside 0 / 1.
 * Workspace: sdrhip_am_bank_workspace_bytes(b, count) bytes for a run of count = k_end - k_begin outputs, 16-byte aligned, used
 * during the run only.  It is what route 2 needs (the complex rows, the envelope rows and dcBlocker's workspace) and is asked for on
 * routes 0 and 2; route 1 asks for the envelope rows and dcBlocker's workspace with dc_block = 1 (a workspace of the full size
 * serves), and for NO workspace with dc_block = 0: d_workspace may then be NULL.
 * Run: SDRHIP_ERR_ARG before any device work, with nothing written, for whatever sdrhip_tuner_bank_run* refuses (its even-stride rule
 * aside: any out_stride >= k_end - k_begin is legal, odd ones included, and any with one channel), out_stride < k_end - k_begin with
 * more than one channel, a null d_dc_state with dc_block = 1 or a non-null one with dc_block = 0, a workspace that is null, shorter
 * than the route asks for or not 16-byte aligned, a d_out off a float's alignment, and route 1 forced on a launch the tuner bank's
 * banked launch does not serve.  An empty range is SDRHIP_OK and leaves the state as it is.  Asynchronous on `stream`; after the first
 * run a run makes no allocation, no host synchronisation and no host-to-device copy on route 1.  An AM bank is immutable after create
 * (but for set_route) and may be shared by host threads.
 * Routes (same bits).  1 = fused: ONE launch of the tuner bank's tile kernel in its envelope form for all channels -- the magnitude of
 * each finished output is what the kernel stores, so no complex row is written or read back -- one envelope fix-up launch for all
 * channels where the tuner bank takes one, and with dc_block = 1 one sdrhip_dc_blocker_run_rows launch set from the envelope rows in
 * the workspace into d_out (that operator refuses d_in == d_out); with dc_block = 0 the tile launch writes d_out itself.  It fits
 * exactly where the tuner bank's banked launch fits (AVX order, factor 4 / 8 / 16, up to 128 prepared taps, seam_block >= 0, a 16-byte
 * aligned first window; d_out needs a float's alignment only) and is SDRHIP_ERR_ARG elsewhere.  2 = composed: the three calls of the
 * definition, the tuner bank on ITS route setting.  0 = auto (default): route 1 where it fits AND the launch lies in the part of the measured
 * rectangle where route 1's slowest round was below route 2's fastest (tools/am_bank_bench.py, profiles/am_bank_bench.txt: 1 / 2 / 8 / 32
 * channels x launches of 8192, 2^17, 2^20 and 2^24 input samples, 128 taps / 8, u8, cfloat and int16 input, dc_block off and on, the two
 * routes alternating in one process, 7 rounds); everything else, and everything outside that rectangle, is route 2.  The rule, with
 * n = (k_end - k_begin) * factor the input samples of the launch, for the three input types alike:
 *     dc_block = 0:  fused  iff  n <= 2^24
 *     dc_block = 1:  fused  iff  n <= 2^24  and  ( channels >= 8  or  channels == 1 and n >= 1048456  or  channels == 2 and n >= 16777096 )
 * Without dcBlocker route 1 is ahead at all 48 measured points, one channel included (0.75 .. 0.91 of route 2's time: 9.2 against
 * 11.5 us for 8 channels at 8192 samples of u8, 921 against 1051 us for 32 channels at 2^24).  With dcBlocker its walk is most of
 * either route (76.9 against 79.3 us for 8 channels at 8192 samples) and route 1 is ahead at all 24 points with 8 and 32 channels
 * (0.89 .. 0.99) but NOT with 1 and 2 channels at 8192 and 2^17 samples: one channel at 8192 samples is BEHIND (43.9 against 37.9 us
 * u8, 41.8 against 37.5 cfloat, 44.2 against 39.6 int16), two channels are 1.01 .. 1.03, at 2^17 the spreads overlap, and two
 * channels at 2^20 are ahead for int16 alone.  One channel at the 2^20 and 2^24 launches and two channels at the 2^24 launch are ahead
 * for every input type, by 0.5 .. 1.9 %, and the rule takes them: 1048456 and 16777096 are those measured launches (131057 and 2097137
 * outputs x 8 samples).  2 < channels < 8 with dcBlocker, and anything beyond 2^24 samples per launch, is not measured and is route 2.
 * Under auto a launch that the envelope kernel turns down after the predicate admitted it runs composed (route 1 forced: an error). */
typedef struct sdrhip_am_bank sdrhip_am_bank;
int sdrhip_am_bank_create(sdrhip_am_bank **b, const sdrhip_tuner_bank *tuner_bank, int dc_block);
void sdrhip_am_bank_destroy(sdrhip_am_bank *b);
int sdrhip_am_bank_channels(const sdrhip_am_bank *b);
int sdrhip_am_bank_set_route(sdrhip_am_bank *b, int route);          /* 0 auto, 1 fused, 2 composed */
size_t sdrhip_am_bank_workspace_bytes(const sdrhip_am_bank *b, int64_t count);   /* 0 for a null bank or a count outside 1 .. 2^31 - 2 */
int sdrhip_am_bank_run(const sdrhip_am_bank *b, void *stream, const float *d_in, int64_t in_base, float *d_out, int64_t out_stride,
                       int64_t k_begin, int64_t k_end, int64_t seam_block, float *d_dc_state, void *d_workspace,
                       size_t workspace_bytes);
int sdrhip_am_bank_run_u8(const sdrhip_am_bank *b, void *stream, const uint8_t *d_in_iq, int64_t in_base, float *d_out,
                          int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, float *d_dc_state,
                          void *d_workspace, size_t workspace_bytes);
int sdrhip_am_bank_run_i16(const sdrhip_am_bank *b, void *stream, const int16_t *d_in_iq, int64_t in_base, float *d_out,
                           int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, float *d_dc_state,
                           void *d_workspace, size_t workspace_bytes);
/* envelope tile launches (route 1: exactly one per run; an int16 one also counts in sdrhip_debug_tuner_i16_launches, none counts in
 * sdrhip_debug_tuner_bank_launches or sdrhip_debug_am_demod_launches) and envelope fix-up launches (at most one per run), process-wide */
long long sdrhip_debug_am_bank_launches(void);
long long sdrhip_debug_am_bank_fixup_launches(void);
/* launches of the all-Cross envelope kernel of the bank's Pipe (sdrhip_pipe_am_bank: the boundary part of a ragged push), process-wide;
 * sdrhip_am_bank_run never takes it */
long long sdrhip_debug_am_bank_cross_launches(void);

/* ---- narrow-band FM demodulator bank: fmDemod of every channel of one capture ---- */
/* The tuner bank with fmDemod (Demod.hs:21-46) as its output form: NOAA weather channels, marine VHF, PMR, 2 m.  "nfm" names the
 * use; the object fixes no bandwidth (that is the tuner bank's decimator) and has no audio stages behind the demodulator.
 * Definition: channel j's row is d_out + j * out_stride floats and holds k_end - k_begin floats; they equal, bit for bit, what
 * sdrhip_tuner_bank_run / _run_u8 / _run_i16 writes into complex rows for the same (d_in, in_base, k_begin, k_end, seam_block), put
 * through sdrhip_fm_demod_run_rows with d_last_iq = d_state and d_last_out = d_final -- on every route, for every seam_block,
 * in_base, cut into launches and out_stride.  Output k is phase(y[k] * conjugate y[k - 1]) of channel j's decimated outputs y.
 * Floats of d_out outside the K rows' [0, k_end - k_begin) are not touched.
 * d_state: K (re, im) pairs of device floats, channel j's decimated output k_begin - 1 at [2j, 2j + 2), read only; NULL = zeros, the
 * start of a stream (Demod.hs:41).  d_final: K pairs that receive every channel's decimated output k_end - 1; NULL = not wanted.
 * THE TWO MUST NOT OVERLAP (the first workgroup of a launch reads one while the last writes the other).  Consecutive runs over
 * consecutive ranges [k0, k1), [k1, k2), ... that swap two state arrays between runs, on one stream, are ONE stream and give the bits
 * of one run over [k0, kn).  Two streams (two host threads on one bank) take two pairs of state arrays and two workspaces.
 * Create: the tuner bank is BORROWED and must outlive the bank; SDRHIP_ERR_ARG (and *b = NULL) for a null tuner bank.
 * Workspace: sdrhip_nfm_bank_workspace_bytes(b, count) bytes for a run of count = k_end - k_begin outputs, 16-byte aligned, used
 * during the run only: route 2's complex rows.  Routes 0 and 2 ask for it; route 1 asks for none (d_workspace may be NULL).
 * Run: SDRHIP_ERR_ARG before any device work, with nothing written, for a null bank, a range outside 0 <= k_begin <= k_end (or of
 * 2^31 - 1 outputs and more), a first window before d_in, seam_block in (0, numCoeffs), out_stride < k_end - k_begin with more than
 * one channel, a d_out (or a state array) off a float's alignment, an int16 input at an address that is no multiple of 4,
 * overlapping state arrays, a workspace that is null, short or not 16-byte aligned on routes 0 and 2, and route 1 forced on a launch
 * it does not serve.  An empty range is SDRHIP_OK and copies d_state (or zeros) to d_final, on every route, as
 * sdrhip_fm_demod_run_rows does.  Asynchronous on `stream`; after the first run a run makes no allocation, no host synchronisation and
 * no host-to-device copy on route 1.  A bank is immutable after create (but for set_route) and may be shared by host threads.
 * Routes (same bits).  1 = fused: exactly ONE launch of the tuner bank's tile kernel in its fmDemod form, for all channels and
 * nothing else -- no complex row is written or read back, no workspace.  Tiles overlap by one thread's pair of outputs so that no
 * workgroup waits on another (2 of 512 outputs are computed twice), and Cross outputs are ALWAYS computed in the tile, for any
 * numCoeffs <= seam_block < 2^30.  It fits where the tuner bank's banked launch fits (AVX order, factor 4 / 8 / 16, up to 128 prepared
 * taps, seam_block >= 0, a 16-byte aligned first window; d_out needs a float's alignment only) with seam_block < 2^30, and is
 * SDRHIP_ERR_ARG elsewhere.  2 = composed: the two calls of the definition, the tuner bank on ITS route setting.  0 = auto (default).
 * Route 1 where it fits AND the launch lies in the part of the measured sweep where route 1's slowest round was below route 2's
 * fastest for all three input types (tools/nfm_bank_bench.py, profiles/nfm_bank_bench.txt: 1 / 2 / 8 / 32 channels x launches of 8192,
 * 2^17, 2^20 and 2^24 input samples, u8 / cfloat / int16, factors 8 and 16, seam_block 0 and 8192, the two routes alternating in one
 * process, 7 rounds); everything else is route 2.  With n = (k_end - k_begin - 1) * factor + numCoeffs the launch's input samples:
 *     factor 8,  seam_block 0:        fused  iff  n <= 2^24
 *     factor 8,  seam_block >= 8192:  fused  iff  n <= 2^20  or  ( channels == 1 and n <= 2^24 )
 *     factor 16, seam_block 0:        fused  iff  n <= 2^24 (channels <= 2),  n <= 2^17 (3 .. 8),  n <= 8192 (9 .. 32)
 *     factor 16, seam_block >= 8192:  fused  iff  n >= 2^17  and  n <= 2^24 (1 channel),  2^20 (2 .. 8),  2^17 (9 .. 32)
 * Factor 8 without seams is ahead at all 48 points (0.63 .. 0.97 of route 2's time: 10.0 against 11.2 us for one channel at 8192
 * samples of u8, 977 against 1045 us for 32 channels at 2^24).  Route 1 is NOT ahead, and auto is route 2: at 2^24 samples with
 * seams and more than one channel (factor 8: 1.06 .. 1.31; factor 16: 1.01 .. 1.49 -- every output pays the in-tile seam test's
 * modulo and whole waves recompute the Cross outputs that route 2's fix-up launch gives one thread each); at factor 16 without seams
 * with 8 channels from 2^20 on and 32 channels from 2^17 on (1.01 .. 1.11 for at least one input type; 32 channels at 2^20 are
 * ahead by 1 .. 2 % between two points that are not, and stay on route 2); at factor 16 with seam_block 8192 at 8192 samples (1.07
 * .. 1.14: 19.6 against 18.0 us) and with 32 channels at 2^20 (1.09 .. 1.20).  A channel count between two measured ones is fused
 * only where both neighbours are.  NOT MEASURED, hence route 2: 0 < seam_block < 8192 (more seams a tile, up to every output Cross),
 * factor 4, more than 2^24 samples a launch; seam_block > 8192 is held to the seam-8192 rows and other tap counts to the rule,
 * unmeasured.  As a reference point the sweep times the AM bank's envelope launch set at the same shapes: the fmDemod form takes
 * 0.90 .. 1.26 of its time at factor 8 without seams (fmDemod is ~100 VALU instructions an output where the magnitude is a few),
 * 0.45 .. 1.58 with seams (the envelope form's fix-up launch against Cross outputs in the tile).  Under auto a launch that the kernel
 * turns down after the predicate admitted it runs composed (route 1 forced: an error). */
typedef struct sdrhip_nfm_bank sdrhip_nfm_bank;
int sdrhip_nfm_bank_create(sdrhip_nfm_bank **b, const sdrhip_tuner_bank *tuner_bank);
void sdrhip_nfm_bank_destroy(sdrhip_nfm_bank *b);
int sdrhip_nfm_bank_channels(const sdrhip_nfm_bank *b);
int sdrhip_nfm_bank_set_route(sdrhip_nfm_bank *b, int route);          /* 0 auto, 1 fused, 2 composed */
size_t sdrhip_nfm_bank_workspace_bytes(const sdrhip_nfm_bank *b, int64_t count);   /* 0 for a null bank or a count outside 1 .. 2^31 - 2 */
int sdrhip_nfm_bank_run(const sdrhip_nfm_bank *b, void *stream, const float *d_in, int64_t in_base, float *d_out, int64_t out_stride,
                        int64_t k_begin, int64_t k_end, int64_t seam_block, const float *d_state, float *d_final, void *d_workspace,
                        size_t workspace_bytes);
int sdrhip_nfm_bank_run_u8(const sdrhip_nfm_bank *b, void *stream, const uint8_t *d_in_iq, int64_t in_base, float *d_out,
                           int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, const float *d_state, float *d_final,
                           void *d_workspace, size_t workspace_bytes);
int sdrhip_nfm_bank_run_i16(const sdrhip_nfm_bank *b, void *stream, const int16_t *d_in_iq, int64_t in_base, float *d_out,
                            int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, const float *d_state, float *d_final,
                            void *d_workspace, size_t workspace_bytes);
/* fmDemod-form tile launches (route 1: exactly one per run; an int16 one also counts in sdrhip_debug_tuner_i16_launches, none counts in
 * sdrhip_debug_tuner_bank_launches, sdrhip_debug_am_bank_launches or sdrhip_debug_rows_launches), process-wide */
long long sdrhip_debug_nfm_bank_launches(void);
/* launches of the all-Cross fmDemod-form kernel of the bank's Pipe (sdrhip_pipe_nfm_bank: the boundary part of a ragged push),
 * process-wide; sdrhip_nfm_bank_run never takes it */
long long sdrhip_debug_nfm_bank_cross_launches(void);

/* ---- narrow-channel bank: a second decimator and the demodulator behind the tuner bank ---- */
/* The AM and narrow-band FM banks demodulate at the tuner bank's output rate, 150 .. 300 ksample/s; the channels they are named for are
 * 8.33 / 12.5 / 25 kHz wide, and a demodulator is non-linear: the noise of the whole band it is fed lands in the audio.  The narrow
 * bank puts a second complex decimator in front of it:   tuner -> firDecimator D1 -> firDecimator D2 -> (magnitude | fmDemod) [-> dcBlocker]
 * Create: tuner_bank and decimator2 are BORROWED and must outlive the bank.  decimator2 is an sdrhip_decimator on complex data
 * (decimateAVXRC and its kin), factor D2, prepared length Lp2 = sdrhip_decimator_num_coeffs.  form: SDRHIP_NARROW_ENV (`magnitude`) or
 * SDRHIP_NARROW_FM (fmDemod); dc_block (dcBlocker behind the envelope) is legal with SDRHIP_NARROW_ENV only.  SDRHIP_ERR_ARG (and
 * *b = NULL) for a null tuner bank, a null decimator, a decimator on real data, a form out of range, dc_block outside 0 / 1 and
 * dc_block with SDRHIP_NARROW_FM.
 * Definition (and route 2): channel j's row is d_out + j * out_stride floats and holds the stage-2 outputs [k_begin, k_end) of
 *   - sdrhip_tuner_bank_run / _run_u8 / _run_i16 over the stage-1 outputs [j_begin, j_end) = [k_begin D2, (k_end - 1) D2 + Lp2)
 *     (sdrhip_narrow_bank_stage1_range; an empty range gives j_begin == j_end) with seam_block, into complex rows of the workspace,
 *   - sdrhip_decimator_run_rows(decimator2, ..., in_base = j_begin, seam_block2, route 0),
 *   - sdrhip_am_demod_run_rows (ENV), or sdrhip_fm_demod_run_rows with d_last_iq = d_state and d_last_out = d_final (FM),
 *   - with dc_block, sdrhip_dc_blocker_run_rows from and to d_dc_state, with a workspace and the default run-in
 * -- bit for bit on every route, for every pair of seam blocks, in_base, cut into consecutive launches and out_stride.  Floats of
 * d_out outside the K rows' [0, k_end - k_begin) are not touched.
 * seam_block is the first decimator Pipe's input block in samples, as sdrhip_tuner_bank_run takes it.  seam_block2 counts STAGE-1
 * OUTPUTS: the first decimator Pipe's output block size, which is the second one's input block; 0 = no seams, otherwise at least Lp2.
 * d_state / d_final: K (re, im) pairs, every channel's STAGE-2 output k_begin - 1 and k_end - 1; SDRHIP_NARROW_FM only (NULL with ENV),
 * NULL is legal, the two must not overlap, and consecutive runs over consecutive ranges that swap them are one stream: the rules of
 * sdrhip_nfm_bank_run.  d_dc_state: 2 K device floats, read and written, with dc_block and NULL without; THE STATE BELONGS TO OUTPUT
 * k_begin, as sdrhip_am_bank_run's does, and consecutive runs that reuse it are one stream.
 * Workspace: sdrhip_narrow_bank_workspace_bytes(b, count) bytes for count = k_end - k_begin outputs, 16-byte aligned, used during the
 * run only: the stage-1 complex rows (16-byte aligned rows, laid out by the object), on routes 0 and 2 the stage-2 complex rows, and
 * with dc_block the envelope rows and dcBlocker's own.  The function answers for the bank's CURRENT route setting: route 1's figure is
 * at most route 2's, a workspace of route 2's size serves every route, and route 0 asks for route 2's because it may fall back.  0 for
 * a null bank, a count outside 1 .. 2^31 - 2 and a count whose stage-1 range has 2^31 - 1 outputs or more.
 * Run: SDRHIP_ERR_ARG before any device work, with nothing written, for whatever the composed calls refuse (a range outside
 * 0 <= k_begin <= k_end, seam_block in (0, numCoeffs), out_stride < k_end - k_begin with more than one channel, an int16 input off a
 * multiple of 4, the tuner bank's route 1 forced on a stage-1 launch it does not serve, ...), a first window before d_in
 * (j_begin D1 < in_base), 0 < seam_block2 < Lp2 (or a negative one), a workspace that is null, short or not 16-byte aligned, state
 * pointers that do not match the form, overlapping state arrays, a d_out or a state array off a float's alignment, and route 1 forced
 * on a shape it does not serve.  An empty range is SDRHIP_OK: with SDRHIP_NARROW_FM it copies d_state (or zeros) to d_final, the dc state
 * is left as it is, no workspace is asked for.  Asynchronous on `stream`; after the first run a run on route 1 makes no allocation, no
 * host synchronisation and no host-to-device copy.  A bank is immutable after create (but for set_route) and may be shared by host
 * threads; two streams take two sets of state arrays and two workspaces.
 * Routes (same bits).  1 = fused: the tuner bank on ITS route setting into the workspace rows, then exactly ONE launch of
 * k_narrow_rows for all channels -- the second decimator with the demodulator as its store: one workgroup per (tile of 256 outputs,
 * channel), the tile's input span staged into LDS with 16-byte loads, one thread per output, a One output summed in decimateAVXRC's
 * order, a Cross output sequentially by the same thread (any number of seams a tile), then `magnitude`, or fmDemod's phase with the
 * predecessor from the neighbouring thread, from an overlap of one output between tiles, or from d_state; the last tile writes
 * d_final.  No stage-2 complex row is written or read back.  With dc_block the sdrhip_dc_blocker_run_rows launch set follows, from
 * envelope rows in the workspace.  It serves the AVX order, D2 <= 16, Lp2 <= 128 and seam_block2 equal to 0 or in [Lp2, 2^30), and is
 * SDRHIP_ERR_ARG elsewhere.  2 = composed: the calls of the definition.  0 = auto (default): route 1 where it fits AND the run lies at
 * points of the measured sweep where route 1's slowest round was below route 2's fastest for all three input types
 * (tools/narrow_bank_bench.py, profiles/narrow_bank_bench.txt: 1 / 2 / 8 / 32 channels x launches of 8192, 2^17, 2^20 and 2^24 input
 * samples through the 128-tap / 8 tuner bank -- 1009 / 16369 / 131057 / 2097137 stage-1 outputs a channel -- u8 / cfloat / int16, the
 * envelope form without and with dcBlocker and the fmDemod form, second decimators 24 taps / 4 and 61 taps / 5, (seam_block,
 * seam_block2) = (0, 0) and (8192, 1024), the two routes alternating in one process, 7 rounds, windows of 0.05 s; 576 points).  The rule
 * is the transcript's closing tables, held as masks in narrow_bank.cpp, over count = k_end - k_begin against the measured launches'
 * 247 / 4087 / 32759 / 524279 outputs a channel (factor 4) and 190 / 3262 / 26199 / 419415 (factor 5): a count at a measured size takes
 * that point, between two measured sizes both neighbours must be ahead, and a channel count between two measured ones takes both
 * neighbours.  Without dcBlocker route 1 is ahead at 120 of the 128 table cells: at every cell up to 2^20 samples
 * (medians 0.35 .. 0.94 of route 2's time: 10.8 against 13.7 us for one channel at 8192 samples of u8, envelope, 24 / 4; 19.8 against
 * 40.9 us for 8 channels at 2^17 samples, fmDemod, 61 / 5, seamed) and NOT at 2^24 samples with 8 and 32 channels at factor 4 (0.97
 * .. 1.04: one thread per output is no faster than the banked tile kernel there).  With dcBlocker its walk is most of either route
 * (0.81 .. 1.08, level from 2^20 samples on) and 49 of 64 cells are ahead.  NOT MEASURED, hence route 2: counts below the smallest or
 * above the largest measured one, more than 32 channels, second factors other than 4 and 5,
 * more prepared taps than the measured decimator of that factor (24, 64; fewer are held to the rule unmeasured), seam_block2 other
 * than 0 and 1024.  seam_block and the tuner bank's own shape are not told apart: stage 1 is the same call on both routes. */
#define SDRHIP_NARROW_ENV 0
#define SDRHIP_NARROW_FM  1
typedef struct sdrhip_narrow_bank sdrhip_narrow_bank;
int sdrhip_narrow_bank_create(sdrhip_narrow_bank **b, const sdrhip_tuner_bank *tuner_bank, const sdrhip_decimator *decimator2, int form,
                              int dc_block);
void sdrhip_narrow_bank_destroy(sdrhip_narrow_bank *b);
int sdrhip_narrow_bank_channels(const sdrhip_narrow_bank *b);
int sdrhip_narrow_bank_set_route(sdrhip_narrow_bank *b, int route);          /* 0 auto, 1 fused, 2 composed */
size_t sdrhip_narrow_bank_workspace_bytes(const sdrhip_narrow_bank *b, int64_t count);
/* host arithmetic: the stage-1 outputs [*j_begin, *j_end) that stage-2 outputs [k_begin, k_end) read */
int sdrhip_narrow_bank_stage1_range(const sdrhip_narrow_bank *b, int64_t k_begin, int64_t k_end, int64_t *j_begin, int64_t *j_end);
int sdrhip_narrow_bank_run(const sdrhip_narrow_bank *b, void *stream, const float *d_in, int64_t in_base, float *d_out, int64_t out_stride,
                           int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t seam_block2, const float *d_state, float *d_final,
                           float *d_dc_state, void *d_workspace, size_t workspace_bytes);
int sdrhip_narrow_bank_run_u8(const sdrhip_narrow_bank *b, void *stream, const uint8_t *d_in_iq, int64_t in_base, float *d_out,
                              int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t seam_block2,
                              const float *d_state, float *d_final, float *d_dc_state, void *d_workspace, size_t workspace_bytes);
int sdrhip_narrow_bank_run_i16(const sdrhip_narrow_bank *b, void *stream, const int16_t *d_in_iq, int64_t in_base, float *d_out,
                               int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t seam_block2,
                               const float *d_state, float *d_final, float *d_dc_state, void *d_workspace, size_t workspace_bytes);
/* launches of k_narrow_rows (route 1: exactly one per run; none counts in sdrhip_debug_fir_rows_launches,
 * sdrhip_debug_am_demod_launches or sdrhip_debug_rows_launches), process-wide */
long long sdrhip_debug_narrow_bank_launches(void);
/* outputs a tile of k_narrow_rows advances by: 256 (ENV), 255 (FM: tiles overlap by one output); 0 for a form out of range */
int sdrhip_debug_narrow_bank_tile(int form);

/* The FIR operators over rows: the filter, decimator and resampler stages behind a bank (second decimator per channel, resampler
 * and audio filter per station) in one launch set instead of one call per row.  in_base, k_begin, k_end, seam_block and out_block
 * mean what they mean to sdrhip_filter_run / sdrhip_decimator_run / sdrhip_resampler_run and are the same for every row; row r's
 * d_in[0] is ITS stream element in_base.  Row r's outputs [k_begin, k_end) equal, bit for bit, what the one-row call writes for
 * that row alone with the same arguments -- on every route, for every rows, stride, in_base and cut into launches, and whatever the
 * other rows hold.  Nothing new is argued: the summation orders, the One / Cross rule and the resampler's two corner cases (a seam
 * without crossover, the late first output of an output block) are the one-row operators'.  Floats of d_out outside the rows'
 * outputs are not touched.  Asynchronous on `stream`; after the descriptor's first run no allocation, no host synchronisation and
 * no host-to-device copy (a row's base and stride travel in the kernel's arguments).  No alignment is asked of bases or strides
 * beyond the element's own.
 * Routes (same bits).  1 = banked: ONE launch of the lane-split tile kernel with the row on the grid's second axis, and ONE fix-up
 * launch for the Cross outputs of all rows when a seam lies inside the range -- whatever rows is.  It serves a SIMD order (SSE / AVX),
 * real or complex data, the symmetric real filters, up to 64 chunks of lane-count taps, resamplers of up to 64 polyphase groups,
 * seam_block >= 0; on anything else (the scalar order, longer filters, more groups, seam_block < 0) it returns SDRHIP_ERR_ARG.
 * There is no minimum length.  2 = row by row: the one-row operator per row on the caller's stream, every shape.  0 = auto: see the
 * rule below; where it does not bank, row by row.
 * SDRHIP_ERR_ARG, before any device work and with nothing written: whatever the one-row call refuses, rows outside
 * 1 .. SDRHIP_ROWS_MAX, a route outside 0 .. 2, and with a non-empty range a null pointer, d_in == d_out, an odd stride on a complex
 * side, with rows > 1 an out_stride shorter than a row's outputs or an in_stride shorter than the inputs the one-row call is
 * guaranteed, counted from in_base (complex: two floats each).  An empty range is SDRHIP_OK and touches nothing.
 * Auto rule.  Auto banks a launch only where the banked route serves the shape AND the launch lies in the part of the measured
 * sweep where the banked call's slowest round was below the K one-row calls' fastest (tools/fir_rows_bench.py,
 * profiles/fir_rows_bench.txt: 1 / 2 / 8 / 32 rows x 128 / 1024 / 16384 / 2^20 outputs per row, 7 rounds; a complex AVX decimator
 * 64 taps / 4, a real AVX resampler 3/10 and a real symmetric AVX filter, each with seam_block 0 and with one seam inside the
 * range).  Those three stand for their family and data type; a real decimator, a complex filter and a complex resampler were not
 * measured and go row by row, as do one row, more than 32 rows and fewer than 128 or more than 2^20 outputs per row.  With n the
 * outputs per row, the fewest rows that are banked at the measured sizes n = 128 / 1024 / 16384 / 2^20:
 *                          seam_block 0          a seam inside the range
 *     complex decimator    2 / 2 / 2 / 8         2 / 8 / 8 / 8
 *     real resampler       2 / 2 / 2 / 2         2 / 8 / 8 / 8
 *     real filter          2 / 2 / 8 / 32        2 / 8 / 8 / 8
 * An n between two measured sizes takes the larger of their two entries; a seam_block > 0 with no seam inside the range takes the
 * larger of the two columns.  Every entry is the smallest measured row count from which all larger ones were ahead (8 where 2 was
 * not, so 3 .. 7 rows wait with it): the crossovers are real -- from 1024 outputs on a seamed one-row call is a single launch of
 * the generic or a specialised kernel (7 .. 40 us for two rows against 12 .. 45 us banked), and at 2^20 outputs the one-row
 * filter kernel is as fast per row as the tile kernel (43 against 45 us for 8 rows).  One row is ahead only at 128 outputs
 * (the decimator, 4.6 against 5.2 us, and the resampler without a seam, 4.2 against 5.9 us), an edge of the sweep, and behind by
 * 1.2x .. 3.1x elsewhere: it stays row by row. */
int sdrhip_filter_run_rows(const sdrhip_filter *f, void *stream, const float *d_in, int64_t in_stride, int64_t in_base,
                           float *d_out, int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block,
                           int route);
int sdrhip_decimator_run_rows(const sdrhip_decimator *d, void *stream, const float *d_in, int64_t in_stride, int64_t in_base,
                              float *d_out, int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block,
                              int route);
int sdrhip_resampler_run_rows(const sdrhip_resampler *r, void *stream, const float *d_in, int64_t in_stride, int64_t in_base,
                              float *d_out, int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block,
                              int64_t out_block, int route);
/* Diagnostics: the tile plan of the banked route for rows of outputs [k_begin, k_end) of a descriptor (kind 0 = sdrhip_filter,
 * 1 = sdrhip_decimator, 2 = sdrhip_resampler).  Host arithmetic, no device.  Returns 1 and fills plan[0 .. 5] = {cycles per tile,
 * tiles per row, independent outputs per lane (1 or 2), outputs per cycle (1; a resampler: its groups), and the cycles per tile
 * and outputs per lane the one-row lane-split kernel plans for ONE such row}; 0 when the banked route does not serve the shape
 * (plan untouched).  A tile holds cycles per tile x outputs per cycle outputs.  The rows plan is the one-row plan capped at the
 * row's own cycles (rounded up to a whole run of lanes), so a long row gets plan[0] == plan[4] and plan[2] == plan[5]. */
int sdrhip_debug_fir_rows_plan(const void *desc, int kind, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block,
                               int *plan /* 6 ints */);
long long sdrhip_debug_fir_rows_launches(void);   /* banked tile launches, process-wide; fix-up launches not counted */
long long sdrhip_debug_fir_rows_fixups(void);     /* banked fix-up launches, process-wide */

/* ---- audio tail: the audio stages behind the AM and narrow-band FM banks, over rows ---- */
/* Every row of real demodulated samples y (the AM bank's envelope, the narrow-band FM bank's phase, 150 .. 300 ksample/s) through
 *     firResampler(block)  >->  firFilter(block)  >->  (* gain)
 * to audio.  The create arguments mean what they mean to sdrhip_fm_chain_create; `block` is the one block size of every Pipe of
 * the tail (0 = contiguous).  The tail owns a real sdrhip_resampler and a symmetric real sdrhip_filter of these arguments and
 * refuses what those two creates refuse, and a block shorter than a stage's filter.
 * Plan functions (host arithmetic, no device): _ready(n_y) = the audio outputs whose whole receptive field lies in y[0, n_y);
 * _first_input(q) = the first y index audio output q reads; _max_halo = the longest receptive field of any output, in y samples;
 * _workspace_bytes(rows, n_y) = what routes 0 and 2 ask for with n_y readable elements per row (0 on bad arguments);
 * _block = the block it was created with; _fused_fits = 1 where route 1 serves this tail, else 0.  The arithmetic is the FM
 * chain's (sdrhip_fm_chain_ready / _max_halo) without its decimator and fmDemod.
 * sdrhip_audio_tail_run_rows: row r's d_y[0] is ITS stream element y_base and n_y elements are readable; audio outputs [q0, q1) of
 * row r go to d_audio + r * audio_stride.  Asynchronous on `stream`; after the first run no allocation, no host synchronisation
 * and no host-to-device copy.  Floats of d_audio outside the rows' outputs are not touched.
 * Routes (same bits).  2 = composed, the DEFINITION: sdrhip_resampler_run_rows(seam_block = block, out_block = block) for
 * z outputs [q0, q1 + numCoeffsF - 1), then sdrhip_filter_run_rows(seam_block = block), then sdrhip_scale_run(gain), the z and
 * filter rows in d_workspace -- the row forms on their banked route wherever it serves the shape, else row by row (not on their
 * auto route: the same launch sets whatever the rows and the length, and their auto rule was read from other shapes).  Nothing new
 * is argued about bits.  1 = fused: ONE launch of k_audio_tail_rows and nothing else, no workspace (a null one is accepted); it
 * serves the FM chain's tail -- ratio 3/10 with 64-float polyphase groups, 64 half-taps, the AVX order -- with block 0 or a block
 * of at least a tile (7314 outputs for 192 prepared resampler taps) and at most 2^28.  0 = auto: the rule below.
 * SDRHIP_ERR_ARG, before any device work and with nothing written: a null handle, rows outside 1 .. SDRHIP_ROWS_MAX, a route
 * outside 0 .. 2, a negative index, and with a non-empty range a receptive field that does not lie in [y_base, y_base + n_y), a
 * null d_y or d_audio, d_y == d_audio, with rows > 1 an audio_stride < q1 - q0 or a y_stride < n_y, on routes 0 and 2 a null
 * workspace or one shorter than _workspace_bytes(rows, n_y), route 1 on a tail it does not serve.  An empty range is SDRHIP_OK
 * and touches nothing.
 * Auto rule.  Auto takes route 1 exactly where it fits AND the run lies at points of the measured sweep where route 1's slowest
 * round was below route 2's fastest (tools/audio_tail_bench.py, profiles/audio_tail_bench.txt: 1 / 2 / 8 / 32 rows x 153 / 2458 /
 * 39322 / 314574 audio outputs per row, block 0 and 8192, the two routes alternating in one process, 7 rounds), in each of three
 * row layouts, which the rule tells apart by the strides: BACK TO BACK (one row, or y_stride == n_y and audio_stride == q1 - q0);
 * Y STRIDED (y_stride != n_y, audio rows back to back -- the audio Pipes' runs: padded y rows behind a carried history; measured
 * with an odd stride and the first row 4 bytes past a 16-byte boundary, so that rows meet the 4-, 8- and 16-byte loaders); AUDIO
 * STRIDED (audio_stride != q1 - q0, where route 2 scales row by row; measured with both sides strided).
 * Route 1 was ahead at all 96 points -- fused / composed, medians: back to back 0.46 .. 0.71 (one row of 153 outputs 6.3 against
 * 13.9 us; 32 rows of 314574 outputs 83 against 180 us with block 0, 115 against 208 us with block 8192), y strided 0.47 .. 0.78
 * (32 rows of 153 outputs 8.1 against 10.7 us, of 314574 outputs 122 against 209 us, block 8192), audio strided 0.07 .. 0.69 (32
 * rows of 2458 outputs 13.9 against 124 us) -- so inside the sweep, 1 .. 32 rows of 153 .. 314574 outputs, auto is route 1 wherever
 * it fits, in every layout, and route 2 everywhere else.  The tables are per layout and block all the same: a run between two
 * measured row counts or sizes is fused only where all its measured neighbours are, a block other than 0 and 8192 must hold in
 * both block tables.  Not measured, hence composed: fewer than 153 or more than 314574 outputs per row, more than 32 rows.  Not
 * measured and not told apart by the rule: strides and offsets other than the three layouts' (a run is classed by which side is
 * strided, not by how far), other blocks than 0 and 8192 that fit, a tile smaller than 2046 outputs. */
typedef struct sdrhip_audio_tail sdrhip_audio_tail;
int sdrhip_audio_tail_create(sdrhip_audio_tail **t, int order, int interpolation, int decimation, const float *resamp_taps,
                             int n_resamp_taps, const float *audio_half_taps, int n_audio_half, float gain, int64_t block);
void sdrhip_audio_tail_destroy(sdrhip_audio_tail *t);
int64_t sdrhip_audio_tail_ready(const sdrhip_audio_tail *t, int64_t n_y);
int64_t sdrhip_audio_tail_first_input(const sdrhip_audio_tail *t, int64_t q);
int64_t sdrhip_audio_tail_max_halo(const sdrhip_audio_tail *t);
int64_t sdrhip_audio_tail_block(const sdrhip_audio_tail *t);
int sdrhip_audio_tail_fused_fits(const sdrhip_audio_tail *t);
/* shape[0 .. 3] = interpolation, decimation, numCoeffsR (the resampler's prepared taps), numCoeffsF (the filter's) */
int sdrhip_audio_tail_shape(const sdrhip_audio_tail *t, int32_t *shape);
size_t sdrhip_audio_tail_workspace_bytes(const sdrhip_audio_tail *t, int rows, int64_t n_y);
int sdrhip_audio_tail_set_route(sdrhip_audio_tail *t, int route);
int sdrhip_audio_tail_run_rows(const sdrhip_audio_tail *t, void *stream, const float *d_y, int64_t y_stride, int64_t y_base,
                               int64_t n_y, float *d_audio, int64_t audio_stride, int rows, int64_t q0, int64_t q1,
                               void *d_workspace, size_t workspace_bytes);
long long sdrhip_debug_audio_tail_launches(void);   /* launches of k_audio_tail_rows (route 1: exactly one per run), process-wide */
/* The general fused kernel, k_audio_tail_rows_any: the same contract and the same bits in ONE launch for every down-sampling ratio a
 * narrow receiver uses (4/5, 3/5, 2/5, 2/3, 3/4, 7/8, 8/9, 1/5, 3/10 ...) with short resamplers and small blocks.  Routes 1 and 2
 * and sdrhip_audio_tail_fused_fits mean what they meant; the general kernel is reached on route 0 only, and only where the rule
 * for route 1 above did not take the run: route 0 decides (1) route 1 by its rule, unchanged, (2) else the general kernel by the
 * mode below, (3) else the composition.  Routes 0 and 2 ask for the workspace whichever way that goes.
 * sdrhip_audio_tail_general_fits: 1 where the general kernel serves this tail, shape and block, else 0 (SDRHIP_ERR_ARG on a null
 * handle).  It serves: real data, resampler and filter in the AVX order, a symmetric filter of at most 128 prepared taps;
 * interpolation <= 8 with gcd(interpolation, decimation) = 1, polyphase groups of at most 64 padded floats, numCoeffsR >=
 * decimation; a tile's y window (840 outputs: decimation * (ceil((840 + numCoeffsF - 1) / interpolation) - 1) + the last group's
 * offset + the group length + 8 floats) within 5120 floats, i.e. decimation / interpolation up to about 5; block 0 or ANY block
 * sdrhip_audio_tail_create admits, up to 2^27 -- a tile may hold any number of buffer boundaries of both stages, so there is no
 * tighter lower bound.
 * sdrhip_audio_tail_set_general(mode), stored as the route is; SDRHIP_ERR_ARG on a null handle or a mode outside 0 .. 2:
 *   0 (default) the measured rule: the general kernel exactly at the points of its sweep where its slowest round was below route
 *               2's fastest (tools/audio_tail_any_bench.py, profiles/audio_tail_any_bench.txt: 1 / 2 / 8 / 32 rows x 51 / 204 / 3276 /
 *               52428 audio outputs per row, block 0 and 256, the three row layouts above, on the tails 4/5 x 63 taps and 2/5 x 127
 *               taps with 2 x 64 audio taps); between measured points every neighbour must be ahead, a block other than 0 and 256
 *               must hold in both block tables, every other tail shape and everything outside the sweep is composed, and a tail of
 *               route 1's shape never takes the general kernel.  The general kernel was ahead at all 192 points -- general / composed,
 *               medians: 4/5 x 63 back to back and y strided 0.37 .. 0.78 (one row of 51 outputs, block 256: 7.6 against 11.3 us;
 *               32 rows of 52428: 52 against 87 us), audio strided 0.05 .. 0.77; 2/5 x 127 back to back and y strided 0.56 .. 0.96
 *               (the closest point: 32 rows of 51 outputs, block 0, 8.9 against 9.3 us), audio strided 0.06 .. 0.87 -- so on those two
 *               tails, 1 .. 32 rows of 51 .. 52428 outputs at any block, mode 0 is the general kernel in every layout.  Not measured,
 *               hence composed: every other ratio, tap count and audio filter length, fewer than 51 or more than 52428 outputs per
 *               row, more than 32 rows;
 *   1           the general kernel wherever it fits;
 *   2           never. */
int sdrhip_audio_tail_general_fits(const sdrhip_audio_tail *t);
int sdrhip_audio_tail_set_general(sdrhip_audio_tail *t, int mode);
long long sdrhip_debug_audio_tail_general_launches(void);   /* launches of k_audio_tail_rows_any, process-wide */

/* ---- the record seam on HOST vectors (hs_sources/SDR/Filter.hs:116-144) ---- */
/* The closures a Haskell constructor puts into the reference's own Filter / Decimator / Resampler records, so that
 * the reference's UNCHANGED Pipes (firFilter / firDecimator / firResampler, Filter.hs:532-727) drive the device:
 *   *_one   = the C SIMD kernel on one buffer: num outputs from in[0 ..] (FilterInternal.hs:66-71,172-177,335-342);
 *   *_cross = the sequential Haskell kernel on `drop i last ++ next` (decimate/filter/resampleCrossHighLevel,
 *             FilterInternal.hs:397-423).
 * HOST pointers, synchronous; n_* in elements (complex pairs for complex descriptors).  The resampler calls carry the
 * reference's state: _one takes the polyphase group and returns the group of the next output (what resampleAVXRR
 * returns), _cross takes the filter offset and returns the offset after the last output; negative = error. */
int sdrhip_filter_one(const sdrhip_filter *f, int num, const float *in, float *out);
int sdrhip_filter_cross(const sdrhip_filter *f, int num, const float *last, int n_last, const float *next, int n_next,
                        float *out);
int sdrhip_decimator_one(const sdrhip_decimator *d, int num, const float *in, float *out);
int sdrhip_decimator_cross(const sdrhip_decimator *d, int num, const float *last, int n_last, const float *next,
                           int n_next, float *out);
int sdrhip_resampler_one(const sdrhip_resampler *r, int group, int num, const float *in, int n_in, float *out);
int sdrhip_resampler_cross(const sdrhip_resampler *r, int filter_offset, int num, const float *last, int n_last,
                           const float *next, int n_next, float *out);
/* Calls of the six above whose buffers were over 512 KiB and went through the copy engine into device buffers instead of being read
 * and written in place from pinned memory; process-wide, for tests that assert which branch a buffer size took. */
long long sdrhip_debug_record_copied_calls(void);

/* ---- the FM receiver chain (examples/fm/fm.hs:34-41) ----------------------- */
/* u8 IQ -> [convert] -> decimator -> fmDemod -> resampler -> symmetric filter
 * [-> * gain].  All four Pipes of fm.hs run with blockSizeOut = block, and the
 * source delivers `block`-sample buffers, so every stage's seams sit at
 * multiples of `block` of its own input index (block = 0: contiguous). */
typedef struct sdrhip_fm_chain sdrhip_fm_chain;
int sdrhip_fm_chain_create(sdrhip_fm_chain **c, int order, int decim_factor, const float *decim_taps,
                           int n_decim_taps, int interpolation, int decimation, const float *resamp_taps,
                           int n_resamp_taps, const float *audio_half_taps, int n_audio_half, float gain,
                           int64_t block);
void sdrhip_fm_chain_destroy(sdrhip_fm_chain *c);
/* Ownership rule for sharding: audio output q is owned by the shard in which its
 * receptive field STARTS.  Given a shard of input samples [s0,s1) of the global
 * stream (plus a right halo), report the owned range [*q0,*q1), and *halo = how
 * many samples past s1 the owned outputs read (the ntaps-1 overlap of every
 * stage composed).  total_in = length of the whole stream (outputs needing data
 * past it do not exist), or -1 for unbounded. */
int sdrhip_fm_chain_plan(const sdrhip_fm_chain *c, int64_t s0, int64_t s1, int64_t total_in,
                         int64_t *q0, int64_t *q1, int64_t *halo);
/* Number of audio outputs whose whole receptive field lies inside the first n_samples samples of the
 * stream, i.e. outputs [0, ready) can be computed from them.  A shard [s0,s1) can compute its outputs
 * [q0, min(q1, ready(s1))) before its halo has arrived. */
int64_t sdrhip_fm_chain_ready(const sdrhip_fm_chain *c, int64_t n_samples);
int64_t sdrhip_fm_chain_max_halo(const sdrhip_fm_chain *c);
size_t sdrhip_fm_chain_workspace_bytes(const sdrhip_fm_chain *c, int64_t n_in);
/* d_in_iq[0] is stream sample s0; n_in samples (shard + halo) are readable.
 * Writes audio outputs [q0,q1) to d_audio[0..q1-q0).  Asynchronous on `stream`. */
int sdrhip_fm_chain_run(sdrhip_fm_chain *c, void *stream, const uint8_t *d_in_iq, int64_t s0, int64_t n_in,
                        float *d_audio, int64_t q0, int64_t q1, void *d_workspace, size_t workspace_bytes);

/* One run with FIXED arguments (pointers, ranges) captured into a hipGraph: a launch-bound batch -- a 2^20-sample shard is
 * nine small kernels -- then costs one graph launch per pass.  Captured from the code path sdrhip_fm_chain_run takes (a
 * plain run precedes the capture: tap uploads and argument checks happen there).  Timing and pipelining must be off. */
typedef struct sdrhip_fm_graph sdrhip_fm_graph;
int sdrhip_fm_chain_graph_create(sdrhip_fm_graph **g, sdrhip_fm_chain *c, const uint8_t *d_in_iq, int64_t s0, int64_t n_in,
                                 float *d_audio, int64_t q0, int64_t q1, void *d_workspace, size_t workspace_bytes);
int sdrhip_fm_chain_graph_launch(sdrhip_fm_graph *g, void *stream);
void sdrhip_fm_chain_graph_destroy(sdrhip_fm_graph *g);

/* Two runs in flight (round 4; default off).  The receiver's successive batches are independent given their raw input
 * (examples/fm/fm.hs:34-41: no stage carries a RESULT from one batch into the next -- only input samples), so with on = 1
 * consecutive sdrhip_fm_chain_run calls alternate between two internal HIP streams and the two halves of the workspace: the
 * memory-heavy tail kernels of run k execute beside the power-bound decimator of run k+1.  Contract while it is on:
 *   - sdrhip_fm_chain_workspace_bytes returns twice the single-run size; pass that much to every run;
 *   - run k starts after everything queued on the caller's `stream` at the time of the call (the producer of its input);
 *   - when the call for run k returns, `stream` has been made to wait for run k-1 -- NOT for run k.  So consecutive runs
 *     must write different audio buffers (double-buffer them), and run k's audio may be consumed on `stream` after the call
 *     for run k+1, or after sdrhip_fm_chain_join(c, stream), which makes `stream` wait for every run still in flight;
 *   - the same holds for run k's INPUT: work queued on `stream` between the calls for run k and run k+1 is ordered after run k-1
 *     only, so the buffer run k reads may be overwritten on `stream` after the call for run k+1 (or after the join) -- double-buffer
 *     the input like the audio;
 *   - results are bit-identical to on = 0 (the same kernels on the same ranges); hipGraph capture needs on = 0.
 * sdrhip_fm_chain_set_overlap drains the runs in flight (host-side wait) before it changes the mode. */
int sdrhip_fm_chain_set_overlap(sdrhip_fm_chain *c, int on);
int sdrhip_fm_chain_join(sdrhip_fm_chain *c, void *stream);
/* fmDemod -> resampler -> audio filter (* gain) as ONE kernel (the demodulated and resampled streams never leave LDS)
 * when the chain has the FM receiver's shape (3/10 resampler with 64-float groups, 64 half-tap symmetric filter, AVX
 * order, buffers longer than one tile).  mode 0 = never (the three stage kernels), 1 = always, 2 = auto (default): only
 * for runs of at most 768 audio outputs (pushes of one or two 8192-sample source blocks), where one launch replaces
 * three; longer runs are faster on the stage kernels (every stage is VALU-bound, and a one-tile run is one workgroup).
 * Same bits. */
int sdrhip_fm_chain_set_fused_tail(sdrhip_fm_chain *c, int mode);
/* launches of that kernel so far, process-wide (tests assert that this path, not the stage kernels or the one-kernel chain, ran) */
long long sdrhip_debug_fused_tail_launches(void);
/* The WHOLE chain (convert + decimator -> fmDemod -> resampler -> audio filter * gain) as ONE kernel for launch-bound runs
 * -- BASELINE configs[4]'s 2^20-sample shard, a push of a few source blocks -- when the chain has the FM receiver's shape
 * (decimation 8 with 128 padded taps, 3/10 resampler with 64-float groups, 64 half-tap symmetric filter, AVX order, 16-byte
 * aligned input whose first sample index is a multiple of 8).  Nothing goes through the workspace; every workgroup recomputes
 * the overlap of its tile (the first stage is computed ~1.9 times over), which pays exactly while a run is bound by launch
 * latency, not by arithmetic.  mode 0 = never, 1 = always, 2 = auto (default): runs of at most max_outputs audio outputs
 * (0 = the built-in bound, 159 * 1728 outputs = ~7.3 M input samples, where the stage kernels catch up: tools/launch_sweep.py).  tile_outputs: audio outputs per workgroup (multiple of 3, at most
 * 159; 0 = chosen from the size of the run: about one workgroup per CU).  Same bits as the stage kernels
 * (examples/fm/fm.hs:34-41; c_sources/decimate.c:105-113, resample.c:70-87, filter.c:60-68; Demod.hs:21-46). */
int sdrhip_fm_chain_set_small_chain(sdrhip_fm_chain *c, int mode, int64_t max_outputs, int tile_outputs);
/* launches of that kernel so far, process-wide (tests assert that this path, not the stage kernels, ran) */
long long sdrhip_debug_small_chain_launches(void);

/* The chain with a tuner: a station that is off the centre of the capture.  Puts `P.map (VG.zipWith (*) osc)` in front of the chain's
 * decimator:  P.map convert >-> P.map (VG.zipWith (*) osc) >-> firDecimator >-> fmDemod >-> firResampler >-> firFilter >-> P.map (* gain).
 * osc_iq = period (re, im) float32 pairs, copied (sdrhip_tuner_shift_table builds the usual ones); period 1 .. 65536; (NULL, 0)
 * removes the tuner again.  SDRHIP_ERR_ARG before any device work for a null chain, a null table with period != 0 (or a table with
 * period 0), a period outside 1 .. 65536 and a non-finite entry.
 * Definition: with t = sdrhip_tuner_create(order, factor, decim_taps, ..., osc_iq, period) the chain's decimator outputs are, bit
 * for bit, what sdrhip_tuner_run_u8(t, ..., seam_block = block) writes; fmDemod, resampler, filter and gain behind them are the
 * chain's as it is, on every route (stage kernels, fused tail, the one-kernel chain).  The oscillator phase of a sample is its
 * ABSOLUTE stream index mod period: it does not depend on s0, on how a stream is cut into runs, shards or pushes, or on `block`,
 * so sdrhip_fm_chain_plan, the halo sizes and exchange, sdrhip_fm_chain_graph_*, sdrhip_fm_chain_set_overlap and sdrhip_fm_stream_*
 * (save / restore included: same state layout) work on a tuned chain as they are.  sdrhip_fm_chain_workspace_bytes of a tuned chain
 * also reserves 8 bytes per input sample (the mixed samples of a launch whose first window is not 16-byte aligned, or whose
 * decimator the tuner's tile kernel does not serve); a chain whose tuner was removed reports and behaves as one that never had one.
 * A large tuned run takes the tuner's tile kernel: the systolic decimator has no tuned form.
 * Call with no run of this chain in flight (after sdrhip_fm_chain_join in overlap mode): the previous table's device copy is
 * freed.  Graphs captured earlier keep what they captured -- the previous table's address included -- and must be destroyed and
 * created again, as must the workspace be re-sized. */
int sdrhip_fm_chain_set_tuner(sdrhip_fm_chain *c, const float *osc_iq, int period);
int sdrhip_fm_chain_tuner_period(const sdrhip_fm_chain *c);      /* 0 = none */
/* launches of the tuned one-kernel chain so far, process-wide (they count in sdrhip_debug_small_chain_launches too) */
long long sdrhip_debug_small_chain_tuned_launches(void);

/* The receiver bank: every station of ONE capture in one launch.  An RTL-SDR capture of 1.28 .. 2.4 Msample/s spans six to twelve
 * broadcast channels; receiving them all with tuned chains is K chains and K runs per push, and the pushes of a live receiver (one
 * to sixteen 8192-sample blocks) are launch-bound: K launch latencies on a chip that is nearly idle during each.  A bank is K tuned
 * chains of the SAME arguments -- chain arguments exactly as sdrhip_fm_chain_create -- with one oscillator table per station:
 * osc_iq[j] = periods[j] (re, im) float32 pairs, copied; 1 .. SDRHIP_FM_BANK_MAX_STATIONS stations; every period 1 .. 65536, every
 * entry finite.  A station on the centre frequency takes the table {1, 0} and is then DEFINED as a chain tuned with that table:
 * there is no untuned station form (the untuned chain folds 1/128 into its taps, a tuned one cannot).
 * Definition: station j's row equals, bit for bit, what a sdrhip_fm_chain created with the same arguments and
 * sdrhip_fm_chain_set_tuner(osc_iq[j], periods[j]) writes for the same (s0, n_in, q0, q1), on every route of the bank and for any
 * tile_outputs.
 * SDRHIP_ERR_ARG before any device work, nothing written: a null handle, 0 or more than 32 stations, a null table pointer, a period
 * outside 1 .. 65536, a non-finite table entry, whatever sdrhip_fm_chain_create refuses, and (sdrhip_fm_bank_run)
 * audio_stride < q1 - q0, a receptive field outside d_in_iq, a workspace too small for the station-by-station route.
 * Like a chain, a bank is created, planned and sized on a host without a GPU; device copies are made by the first run.  More than
 * 32 stations: two banks. */
#define SDRHIP_FM_BANK_MAX_STATIONS 32
typedef struct sdrhip_fm_bank sdrhip_fm_bank;
int sdrhip_fm_bank_create(sdrhip_fm_bank **b, int order, int decim_factor, const float *decim_taps, int n_decim_taps,
                          int interpolation, int decimation, const float *resamp_taps, int n_resamp_taps,
                          const float *audio_half_taps, int n_audio_half, float gain, int64_t block,
                          int stations, const float *const *osc_iq, const int *periods);
void sdrhip_fm_bank_destroy(sdrhip_fm_bank *b);
int sdrhip_fm_bank_stations(const sdrhip_fm_bank *b);
int sdrhip_fm_bank_period(const sdrhip_fm_bank *b, int station);
/* what the tuned chain of the same arguments reports (plan / ready / max_halo do not depend on a table; workspace_bytes is the
 * tuned chain's figure: the station-by-station route runs the stations one after the other on ONE workspace) */
int sdrhip_fm_bank_plan(const sdrhip_fm_bank *b, int64_t s0, int64_t s1, int64_t total_in, int64_t *q0, int64_t *q1, int64_t *halo);
int64_t sdrhip_fm_bank_ready(const sdrhip_fm_bank *b, int64_t n_samples);
int64_t sdrhip_fm_bank_max_halo(const sdrhip_fm_bank *b);
size_t sdrhip_fm_bank_workspace_bytes(const sdrhip_fm_bank *b, int64_t n_in);
/* d_in_iq[0] is stream sample s0, n_in samples are readable (as sdrhip_fm_chain_run).  Station j's audio outputs [q0, q1) go to
 * d_audio + j * audio_stride (floats), audio_stride >= q1 - q0; floats of d_audio outside the K rows' [0, q1 - q0) are not
 * touched.  Asynchronous on `stream`.  After the first run of a shape a run makes no allocation, no host synchronisation and no
 * host-to-device copy: what changes from launch to launch (each station's oscillator phase at the launch's first sample, the row
 * stride) travels in the kernel's arguments.  The banked route sends nothing through the workspace and accepts a null one; the
 * station-by-station route needs sdrhip_fm_bank_workspace_bytes(n_in) bytes.  No overlap mode and no hipGraph helper for a bank;
 * its host-block front end is sdrhip_fm_stream_create_bank (below, with the chain's). */
int sdrhip_fm_bank_run(sdrhip_fm_bank *b, void *stream, const uint8_t *d_in_iq, int64_t s0, int64_t n_in,
                       float *d_audio, int64_t audio_stride, int64_t q0, int64_t q1, void *d_workspace, size_t workspace_bytes);
/* Routes.  1 = the banked launch: ONE launch of the tuned one-kernel chain (sdrhip_fm_chain_set_small_chain) with a station axis in
 * its grid; it fits exactly where that kernel serves a tuned chain -- decimation 8 with 128 padded taps, AVX order, the FM
 * receiver's tail, block 0 or 192 .. 2^26, 16-byte aligned input, s0 a multiple of 8 -- and the grid exists (at most 65535 tiles);
 * forced outside these conditions, sdrhip_fm_bank_run returns SDRHIP_ERR_ARG.  2 = station by station: sdrhip_fm_chain_run of the
 * bank's own tuned chains, one after the other on the caller's stream and workspace.  0 = auto (default), a rule in two
 * dimensions: the banked launch where it fits while a station's run is short, q1 - q0 <= 39322 (a run of 2^20 samples; fixed), AND
 * stations * (q1 - q0) <= max_outputs (0 = the built-in bound, 32 * 39322); else station by station -- every size and alignment
 * the banked launch refuses, and every longer run, whatever the number of stations: those are bound by arithmetic, not by launches,
 * and from 159 * 1728 outputs on a station's own chain leaves the one-kernel route.  Both bounds are the edges of what was measured
 * against K runs of K tuned chains (1 .. 32 stations x runs of up to 2^20 samples), not crossovers.  tile_outputs as
 * sdrhip_fm_chain_set_small_chain (0 = chosen from the total work, stations * outputs).  Same bits on every route. */
int sdrhip_fm_bank_set_route(sdrhip_fm_bank *b, int route, int64_t max_outputs, int tile_outputs);
/* banked launches so far, process-wide (they do NOT count in sdrhip_debug_small_chain_launches: those are the chains') */
long long sdrhip_debug_fm_bank_launches(void);
/* The bank on 16-bit signed IQ (the BladeRF's samples, as sdrhip_tuner_run_i16): d_in_iq is interleaved (I, Q) int16, 4 bytes per
 * sample, d_in_iq[0 .. 1] is stream sample s0; a sample is converted first, (float)s * 2^-11 (exact in float32 over the whole int16
 * range), then mixed.  The SAME bank object serves u8 and int16 runs: plan, ready, max_halo and workspace_bytes are the bank's.
 * Definition: station j's row equals, bit for bit, on every route and for any tile_outputs, the composition
 *     sdrhip_tuner_run_i16 -> sdrhip_fm_demod_run -> sdrhip_resampler_run -> sdrhip_filter_run -> sdrhip_scale_run
 * driven by hand on the same (s0, n_in, q0, q1): a tuner of the bank's decimator arguments with table j, every later stage with the
 * bank's arguments, all of them with the bank's block as their seam block.  A bank of one station with the table {1, 0} is the
 * plain FM receiver on int16 input (the product of a converted sample with 1 + 0i keeps its bits: converted int16 holds no -0 and
 * no subnormal).
 * Routes (sdrhip_fm_bank_set_route; the same setting serves both input types).  1 = the banked launch: ONE launch of the tuned
 * one-kernel chain with a station axis and an int16 loader; it fits where the u8 banked launch fits, under int16's alignment rule:
 * d_in_iq 16-byte aligned and s0 a multiple of 4 (u8: 8).  It accepts a null workspace.  The zero tap that create padded is skipped
 * only while 16 (|re| + |im|) is finite in float32 for every table entry of every station (converted int16 reaches |x| = 16; the
 * u8 run's condition is |re| + |im|).  2 = station by station: the bank's own tuned chains with the tuner's int16 first stage
 * (sdrhip_tuner_run_i16's two routes: its tile kernel where the first window is 16-byte aligned, else the int16 mix into the
 * workspace and the cfloat decimator), everything behind it the code a u8 run takes.  0 = auto: the u8 rule, the banked launch
 * where it fits while q1 - q0 <= 39322 and stations * (q1 - q0) <= max_outputs.  The int16 sweep confirms the u8 rectangle
 * (tools/fm_bank_bench.py --i16, profiles/fm_bank_i16_bench.txt: 2 .. 32 stations x runs of 1 block, 16 blocks and 2^20 samples,
 * the banked launch against route 2 of the same bank): at every point the banked launch's slowest round is below route 2's
 * fastest (0.016 .. 0.27 of its time); with one station it is 0.39 .. 0.50.
 * SDRHIP_ERR_ARG before any device work, nothing written: whatever sdrhip_fm_bank_run refuses, d_in_iq not 4-byte aligned, route 1
 * forced where the banked launch does not fit.  There is no sdrhip_fm_chain_run_i16: int16 reaches the FM side through a bank. */
int sdrhip_fm_bank_run_i16(sdrhip_fm_bank *b, void *stream, const int16_t *d_in_iq, int64_t s0, int64_t n_in,
                           float *d_audio, int64_t audio_stride, int64_t q0, int64_t q1, void *d_workspace, size_t workspace_bytes);
/* banked launches on int16 input so far, process-wide (each of them counts in sdrhip_debug_fm_bank_launches too) */
long long sdrhip_debug_fm_bank_i16_launches(void);
/* launches of the thread-per-polyphase-cycle resampler (real I/D with an odd decimation: 2/3, 5/7, ...; any filter length),
 * process-wide (tests assert that this kernel, not the lane-split one, served those ratios) */
long long sdrhip_debug_resample_cycle_launches(void);
/* launches of the real decimator kernel for factors 2 / 4 / 8 / 16 (kernels_decimate_real.hip), process-wide */
long long sdrhip_debug_decimate_real16_launches(void);
/* Which kernel serves the decimate-by-8, 128-tap, AVX-order first stage: 0 = the LDS-tiled kernel everywhere, 1 = the
 * register-resident systolic kernel (kernels_systolic.hip) wherever its shape fits, in its round-5 form (non-temporal loads, seam
 * fix-up as a second launch), 2 (default; SDRHIP_SYSTOLIC sets the initial value) = the library's own choice: the systolic kernel
 * with the seam fix-up's workgroups inside its launch and plain / non-temporal loads by launch size (tools/route_sweep_fine.py).
 * Results are identical.
 * sdrhip_debug_systolic_launches: launches the systolic kernel has served, process-wide; sdrhip_debug_systolic_plan: the strip cut of a
 * launch of `count` outputs (host arithmetic only): strips [0, nwhole) take the unguarded body. */
void sdrhip_debug_set_systolic(int mode);
long long sdrhip_debug_systolic_launches(void);
void sdrhip_debug_systolic_plan(int count, int *nstrips, int *nwhole);
/* sdrhip_debug_systolic_plain_launches: systolic launches on cfloat input that took plain loads (the mid-size range that the Infinity
 * Cache serves) instead of non-temporal ones; sdrhip_debug_decimator_crossfix_launches: seam fix-ups of the complex AVX-order
 * decimator that ran as a launch of their own after the main kernel (not inside it).  Both process-wide, for tests that assert
 * which route a launch size took. */
long long sdrhip_debug_systolic_plain_launches(void);
long long sdrhip_debug_decimator_crossfix_launches(void);
/* fmDemod inside the resampler's tile loader for large batches (>= 2^18 resampler outputs per run): the demodulated stream
 * never makes its round trip through HBM (12 B per decimated sample less traffic); the per-stage timing then books the pair
 * under `resample` (and reports 0 for `fm_demod`).  Same bits.  ON by default since round 4 (SDRHIP_FUSE_DEMOD=0 turns it off):
 * the pair takes 0.269 ms against 0.159 + 0.089 for the two stage kernels -- the arithmetic is the same -- but the chip runs at its
 * power cap and 0.54 GB less traffic per pass leaves the decimator 4 % more clock: the whole pass gains 1.0 %. */
int sdrhip_fm_chain_set_demod_fusion(sdrhip_fm_chain *c, int enable);
/* resampler launches that took fmDemod into their tile loader, process-wide (the per-stage timing books fmDemod under `resample`
 * whenever the fusion is on, also when a launch too small for the fused form ran a stand-alone fmDemod first: this tells the two apart) */
long long sdrhip_debug_fused_demod_launches(void);
/* u8 launches of a complex filter / decimator that went to the generic kernel (convert, then the plain taps), process-wide: the shapes
 * no u8-fused tiled kernel serves, and every descriptor with a nonzero tap below 2^-119, whose taps / 128 would not be exact. */
long long sdrhip_debug_generic_u8_launches(void);
/* Per-stage timing with HIP events recorded around each stage's kernels on the stream they are
 * launched on; stages {decimate(+seam fix-up), fmDemod, resample, filter(+gain), fused tail (the three in one kernel),
 * whole chain in one kernel (sdrhip_fm_chain_set_small_chain)}.
 * read_timing waits for the recorded runs, returns the SUM of elapsed ms per stage over
 * `*runs` runs and resets the recorder. */
int sdrhip_fm_chain_enable_timing(sdrhip_fm_chain *c, int enable);
int sdrhip_fm_chain_read_timing(sdrhip_fm_chain *c, double ms_sum[6], int *runs);

/* ---- multi-GPU: the ntaps-1 halo exchange of the sharded chain ---- */
/* The reference has no multi-device code; these entry points are what a sharded host (one thread or process per
 * GPU -- e.g. eight Haskell pipelines of examples/fm/fm.hs:34-41, one per device) binds to.  Rank r owns the samples
 * [r*S, (r+1)*S) of every super-block in a device buffer laid out [shard | halo region]; one exchange sends the FIRST
 * `bytes` of the shard to the LEFT neighbour (rank r-1, wrapping) and receives the right neighbour's head into the halo
 * region.  Transport: RCCL point-to-point (ncclGroupStart; ncclSend; ncclRecv; ncclGroupEnd) enqueued on the caller's HIP
 * stream -- librccl.so.1 is loaded on first use, the library has no link-time dependency on it -- or, for the devices of
 * ONE process, hipMemcpyPeerAsync.  The message is ~8 KB: latency-bound, so no collective is involved. */
typedef struct sdrhip_comm sdrhip_comm;
#define SDRHIP_COMM_ID_BYTES 128
/* rank 0 creates the rendezvous id and hands it to the other ranks by any out-of-band means (file, socket, MPI ...) */
int sdrhip_comm_get_unique_id(void *id /* SDRHIP_COMM_ID_BYTES */);
/* one communicator per GPU process / thread; binds the CURRENT device (sdrhip_set_device first).  Collective: every
 * rank must call it. */
int sdrhip_comm_init_rank(sdrhip_comm **c, int nranks, int rank, const void *id);
/* all `ndev` devices from ONE process: comms[i] is rank i on devices[i].  transport: SDRHIP_TRANSPORT_RCCL or
 * SDRHIP_TRANSPORT_PEER_COPY (hipMemcpyPeerAsync; no RCCL needed). */
#define SDRHIP_TRANSPORT_RCCL 1
#define SDRHIP_TRANSPORT_PEER_COPY 2
int sdrhip_comm_init_local(sdrhip_comm **comms, int ndev, const int *devices, int transport);
void sdrhip_comm_destroy(sdrhip_comm *c);
int sdrhip_comm_rank(const sdrhip_comm *c);
int sdrhip_comm_size(const sdrhip_comm *c);
const char *sdrhip_comm_transport(const sdrhip_comm *c);   /* "rccl" | "peer-copy" */
/* One rank's exchange, asynchronous on `stream` (the compute stream: kernels queued after it see the halo).  d_send /
 * d_recv are device pointers on this rank's GPU.  RCCL transport only (a per-rank call cannot see the peer's memory). */
int sdrhip_halo_exchange(sdrhip_comm *c, void *stream, const void *d_send, void *d_recv, size_t bytes);
/* All ranks of a single-process communicator at once: rank i sends d_send[i] and receives into d_recv[i] on streams[i].
 * RCCL: one group over every rank; peer copy: stream i waits for the event of rank i+1's stream (the head must have been
 * produced) and pulls it with hipMemcpyPeerAsync. */
int sdrhip_halo_exchange_all(sdrhip_comm *const *comms, int ndev, void *const *streams, const void *const *d_send,
                             void *const *d_recv, size_t bytes);
/* The chain's own message: head = d_buf[0 .. 2*halo), halo region = d_buf + 2*shard_samples, halo =
 * sdrhip_fm_chain_halo_samples(chain) (max_halo rounded up to 8 samples: the same on every rank). */
int64_t sdrhip_fm_chain_halo_samples(const sdrhip_fm_chain *c);
int sdrhip_fm_chain_halo_exchange(const sdrhip_fm_chain *chain, sdrhip_comm *comm, void *stream, uint8_t *d_buf,
                                  int64_t shard_samples);
/* The halos of `count` consecutive super-blocks in ONE message pair (round 5): the rank's shard of super-block k lies at
 * d_buf + k * row_bytes (head at +0, halo region at + 2 * shard_samples, as above).  The heads are gathered into d_staging
 * (hipMemcpy2DAsync), one ncclSend / ncclRecv of count * 2 * halo bytes moves them, and the received ones are scattered into the
 * halo regions -- all on `stream`.  A launch-bound shard (2^20 samples: ~11 us per pass) cannot hide a point-to-point round trip
 * per pass; with count passes per exchange the round trip is paid once per count passes at the price of count super-blocks
 * being resident before the first is processed.  d_staging:
 * sdrhip_fm_chain_halo_staging_bytes(chain, count) bytes of device memory (a send and a receive half). */
size_t sdrhip_fm_chain_halo_staging_bytes(const sdrhip_fm_chain *chain, int count);
int sdrhip_fm_chain_halo_exchange_batch(const sdrhip_fm_chain *chain, sdrhip_comm *comm, void *stream, uint8_t *d_buf,
                                        int64_t shard_samples, size_t row_bytes, int count, void *d_staging);

/* Host-block streaming front end of the chain: u8 IQ source blocks in (host memory, `block` samples
 * each or a whole multiple), audio blocks of exactly block_size_out floats out -- the five middle
 * stages of examples/fm/fm.hs:34-41 as ONE operator with every intermediate resident in HBM.  Pinned
 * staging in slots = submissions in flight: two when max_block_samples is too large to run in place (results lag one push;
 * H2D / compute / D2H on three HIP streams), four when even the largest push runs on one stream -- up to 200 source blocks: one compute
 * stream per slot; a lone source block is read by the kernel straight from the pinned buffer over PCIe, anything larger (a push of several
 * blocks, or pushes that piled up while the GPU was busy) crosses the link ONCE by a copy on the slot's stream and is then ONE kernel on
 * device memory; the audio is written to the pinned result buffer by the kernel either way (SDRHIP_STAGE_SAMPLES moves the bound) --
 * and results lag three pushes (flush drains; SDRHIP_STREAM_SLOTS=2..4 overrides the count).
 * The chain must outlive the stream and must not be run concurrently by another caller. */
typedef struct sdrhip_fm_stream sdrhip_fm_stream;
int sdrhip_fm_stream_create(sdrhip_fm_stream **st, sdrhip_fm_chain *chain, int max_block_samples, int block_size_out);
void sdrhip_fm_stream_destroy(sdrhip_fm_stream *st);
/* returns the number of complete audio blocks ready to pop (>= 0) or a negative error */
int sdrhip_fm_stream_push(sdrhip_fm_stream *st, const uint8_t *iq, int n_samples);
/* Zero-copy variant: the pinned staging buffer (2*max_block_samples bytes) the NEXT push will upload
 * from.  Let the source (e.g. the RTL-SDR read of SDR/RTLSDRStream.hs) write into it, then push that
 * same pointer: the host-side memcpy is skipped.  Valid until that push; NULL on error.  (With
 * coalescing it points just past the samples already staged; there is always room for
 * max_block_samples more.) */
uint8_t *sdrhip_fm_stream_input_buffer(sdrhip_fm_stream *st);
int sdrhip_fm_stream_flush(sdrhip_fm_stream *st);
/* Audio blocks ready to pop, after collecting (without waiting) every in-flight submission the GPU has finished: lets a
 * real-time caller fetch the audio of the push it just made some tens of microseconds later instead of at its next push
 * (pushes themselves collect finished work too; flush waits for all of it). */
int sdrhip_fm_stream_poll(sdrhip_fm_stream *st);
/* Latency / throughput knob: stage pushes in the pinned buffer and submit them to the GPU together once
 * `samples` samples (a multiple of the chain's block; 0 = every push, the default) have accumulated, or on
 * flush.  One 8192-sample push costs ~8-9 us (one kernel launch, four pushes in flight) whatever its size, so a caller
 * that must keep the reference's block size (fm.hs:17) gets ~6x the throughput from coalesce = 16 blocks, at 16 blocks
 * of latency; the audio blocks are the same.  Call with nothing staged. */
int sdrhip_fm_stream_set_coalesce(sdrhip_fm_stream *st, int samples);
/* The same knob turned by the GPU itself: with max_samples > 0 (a multiple of the chain's block, at least two pushes) a push
 * is submitted at once while the slot its submission would move on to is free, and staged behind the earlier ones while that
 * slot is still running -- up to max_samples, then the push waits.  A source slower than the GPU (a radio) sees every push
 * go out immediately; a faster one (file replay) sees its pushes leave as fewer, larger launches.  Which push returns which
 * audio block then depends on timing; the blocks themselves do not.  0 switches it off.  Call with nothing staged. */
int sdrhip_fm_stream_set_adaptive(sdrhip_fm_stream *st, int max_samples);
int sdrhip_fm_stream_pop(sdrhip_fm_stream *st, float *out, int capacity);
/* A stream over a bank: u8 IQ source blocks in, audio blocks of exactly block_size_out floats out for EVERY station, in lockstep.
 * Same object type as sdrhip_fm_stream_create gives: push, input_buffer, flush, poll, set_coalesce, set_adaptive, state_bytes,
 * save, restore and destroy are the same calls and mean the same; counts they return are blocks PER STATION.
 * Definition: station j's blocks are, bit for bit, those of a sdrhip_fm_stream over a tuned chain of the bank's arguments with
 * table j, fed the same samples -- whatever the push sizes, coalescing, adaptive submission or route.
 * Refused like sdrhip_fm_stream_create and at the same point, before any device work: a null argument, max_block_samples not a
 * multiple of the seam block, block_size_out <= 0.
 * A submission is ONE run of the bank on [carried tail | staged samples]: the bank's own rule (sdrhip_fm_bank_set_route) picks
 * the banked launch or station by station, so a push of more than 39322 outputs per station goes station by station; a run the
 * bank refuses (route 1 where the banked launch does not fit) makes the push fail with nothing written and nothing to pop.
 * Slots, the default adaptive cap and the SDRHIP_* knobs are the chain stream's.  Routes: a stream of more than one station NEVER
 * runs in place -- with K stations in the grid every station's workgroups would fetch the same tile over the link, K times the
 * traffic -- so every submission up to the direct bound is one copy on the slot's stream and one launch on device memory, a lone
 * source block included.  Measured (tools/fm_bank_stream_bench.py, profiles/fm_bank_stream_bench.txt: lone-block pushes, in place
 * against the copy, 2 / 4 / 8 / 12 stations): at no K is in place ahead of the copy by more than the spread of the rounds -- its
 * medians are lower (4.2 .. 4.7 against 5.9 .. 8.8 us per push), but every in-place series holds a round slower than the copy's
 * fastest -- so no in-place region is kept.  A one-station bank's stream follows the chain's rule.
 * The bank must outlive the stream and must not be run by another caller meanwhile. */
int sdrhip_fm_stream_create_bank(sdrhip_fm_stream **st, sdrhip_fm_bank *bank, int max_block_samples, int block_size_out);
/* A bank's stream on 16-bit signed IQ: interleaved int16 source blocks in (4 bytes per sample), every station's audio blocks out.
 * The object sdrhip_fm_stream_create_bank gives, and the same calls with the same meaning: flush, poll, set_coalesce, set_adaptive,
 * pop, pop_rows, rows, state_bytes, save, restore, destroy.  Samples go in through sdrhip_fm_stream_push_i16 and
 * sdrhip_fm_stream_input_buffer_i16 (max_block_samples int16 pairs are writable); the wrong push or input_buffer call for a
 * stream's input type is refused (SDRHIP_ERR_ARG / NULL) with nothing staged.  A submission is ONE sdrhip_fm_bank_run_i16 on
 * [carried tail | staged samples]; the tail starts at a multiple of 8 samples, so the run is 16-byte aligned on the device.
 * Definition: station j's blocks are those of sdrhip_fm_bank_run_i16's composition run over the whole stream -- whatever the push
 * sizes, coalescing, adaptive submission or route.
 * An int16 stream NEVER reads its input in place, whatever the station count: every submission up to the direct bound is one copy
 * on the slot's stream and one run on device memory.  This is a stated choice, not a measured one (for one station it differs from
 * the u8 stream's rule).
 * A state of an int16 stream has a version of its own: it carries the input type, the station count and the history as int16.
 * restore refuses an int16 state on a u8 stream and the reverse; the states of u8 streams keep every byte. */
int sdrhip_fm_stream_create_bank_i16(sdrhip_fm_stream **st, sdrhip_fm_bank *bank, int max_block_samples, int block_size_out);
int sdrhip_fm_stream_push_i16(sdrhip_fm_stream *st, const int16_t *iq, int n_samples);
int16_t *sdrhip_fm_stream_input_buffer_i16(sdrhip_fm_stream *st);
int sdrhip_fm_stream_rows(const sdrhip_fm_stream *st);      /* 1 for a chain's stream, the number of stations for a bank's */
/* Pops up to max_blocks complete audio blocks of every station: station j's nb * block_size_out floats go to
 * out + j * row_stride (row_stride >= max_blocks * block_size_out is checked before anything is written).
 * Returns nb >= 0.  Works on a chain's stream too (one row).  sdrhip_fm_stream_pop keeps its meaning on streams of one row (a bank
 * of one station included); on a stream of more rows it returns SDRHIP_ERR_ARG and pops nothing. */
int sdrhip_fm_stream_pop_rows(sdrhip_fm_stream *st, float *out, int64_t row_stride, int max_blocks);
/* Checkpoint / resume.  Between two pushes the operator's state is the stream position, the last ~4k input samples and
 * the audio not yet popped (the reference keeps the equivalent in Pipe closures: overlap remainder, resampler phase, last
 * demod sample, output fill level -- Filter.hs:536-727, Demod.hs:21-38); everything else is a closed form of the position.
 * state_bytes: drains the operator (like flush) and returns the exact size the save that follows needs (0 = the drain failed);
 * save: drains the operator and writes the state (*used = its size);
 * restore: into a freshly created stream over a chain of the same taps and block sizes; returns the number of audio blocks
 * ready to pop.  A restored stream fed the remaining samples yields the audio the uninterrupted stream would have.
 * A stream of several stations saves a state of its own version that carries the station count and, per station, the audio not
 * yet popped (the same count for every station); a one-row stream's state is byte for byte what it always was.  A state is
 * refused (SDRHIP_ERR_ARG, nothing changed) by a stream whose station count, block_size_out, seam block or halo differs.
 * Oscillator tables are no part of a state: a station's phase is a closed form of the position. */
size_t sdrhip_fm_stream_state_bytes(sdrhip_fm_stream *st);   /* not const: it drains (submits, waits, moves results) */
int sdrhip_fm_stream_save(sdrhip_fm_stream *st, void *buf, size_t capacity, size_t *used);
int sdrhip_fm_stream_restore(sdrhip_fm_stream *st, const void *buf, size_t bytes);

/* ---- spectrum path (hs_sources/SDR/FFT.hs:44-168) on hipFFT ---- */
/* fftw' / fftw (complex-to-complex forward DFT of n Complex Double), fftwReal' / fftwReal (n Double -> n/2+1 bins) and
 * fftwParallel (several buffers in flight: here a batched plan).  Double precision, unnormalised, forward sign
 * exp(-2 pi i jk/n): FFTW's conventions and bin order.  Tolerance contract (a different summation tree from FFTW's), not
 * bit parity.  libhipfft.so.0 is loaded on first use. */
typedef struct sdrhip_fft sdrhip_fft;
int sdrhip_fft_create(sdrhip_fft **f, int n, int real_input, int batch);
void sdrhip_fft_destroy(sdrhip_fft *f);
int sdrhip_fft_size(const sdrhip_fft *f);
int sdrhip_fft_bins(const sdrhip_fft *f);                                  /* n, or n/2 + 1 for real input */
/* HOST vectors, synchronous: in = batch x n complex doubles (interleaved) or batch x n doubles; out = batch x bins complex */
int sdrhip_fft_run(sdrhip_fft *f, const double *in, double *out);
/* DEVICE vectors, asynchronous on `stream` */
int sdrhip_fft_run_device(sdrhip_fft *f, void *stream, const double *d_in, double *d_out);

/* The spectrum operator: the reference's waterfall pipe, interleavedIQUnsigned256ToFloat (Util.hs:92-98) -> halfBandUp
 * (Util.hs:264-271) x hanning / hamming / blackman (FilterDesign.hs:39-60) -> fftw (FFT.hs:44-76) -> magnitude and a scale, from raw
 * IQ (u8, float32 or int16: SDRHIP_IQ_*) in device memory to plot-ready float32 rows.  With x[j] the converted sample, all arithmetic in double:
 *     x'[j] = x[j] * (half_band_shift ? (-1)^j : 1) * w[j];  X = forward DFT of x' (unnormalised, sign exp(-2 pi i jk/n));
 *     out[k] = (float)(scale * |X[k]|),  |X| = sqrt(re^2 + im^2): cf32 input must stay well inside double's range (|x| < 1e150).
 * The windows are computed on the host in double with the reference's formulas (denominator n - 1, so n >= 2).  Tolerance
 * contract, like sdrhip_fft: every bin within 1e-11 of the row's largest bin plus one float32 unit in the last place.
 * Routes: power-of-two n from 64 to 8192 (8192 included: its 128 KiB of LDS fit one workgroup) run as ONE kernel, raw IQ in,
 * magnitudes out, the transform resident in LDS; every other n takes pre-kernel -> hipFFT -> post-kernel through a bounded scratch
 * buffer.  `auto` picks per n the route that measured faster.  Without libhipfft, create succeeds and the one-kernel
 * sizes run; a run on the hipFFT route returns the error sdrhip_fft_create gives.  One object serves one caller at a time. */
typedef struct sdrhip_spectrum sdrhip_spectrum;
#define SDRHIP_IQ_U8   0   /* interleaved unsigned bytes, (v - 128) / 128   (Util.hs:92-98)  */
#define SDRHIP_IQ_CF32 1   /* interleaved float32 re, im (e.g. a decimator's output)          */
/* interleaved int16 (I, Q), c(s) = (double)s * 2^-11 over the WHOLE int16 range (the BladeRF conversion, convert.c:52-85; exact, so it
 * equals (double)((float)s * 2^-11): a cf32 object on sdrhip_convert_i16_run's floats gives the same bits on the one-kernel route).
 * d_in must be 2-byte aligned, else SDRHIP_ERR_ARG before any launch with nothing written; a 4-byte aligned base is read with one load
 * per sample, any other with two.  No byte outside [0, 4 * n_samples) of d_in is read. */
#define SDRHIP_IQ_I16  2
#define SDRHIP_WINDOW_NONE 0
#define SDRHIP_WINDOW_HANNING 1    /* FilterDesign.hs:39-44 */
#define SDRHIP_WINDOW_HAMMING 2    /* :47-52 */
#define SDRHIP_WINDOW_BLACKMAN 3   /* :55-60 */
#define SDRHIP_WINDOW_CUSTOM 4     /* n doubles from the caller */
int  sdrhip_spectrum_create(sdrhip_spectrum **s, int n, int input_format, int window, const double *custom_window,
                            int half_band_shift, double scale);
void sdrhip_spectrum_destroy(sdrhip_spectrum *s);
int  sdrhip_spectrum_size(const sdrhip_spectrum *s);
int  sdrhip_spectrum_window(const sdrhip_spectrum *s, double *out /* n */);   /* the window in use */
/* row r = samples [r*hop, r*hop + n) of d_in; needs hop >= 1 and (rows-1)*hop + n <= n_samples, else SDRHIP_ERR_ARG.
 * d_out: rows x n float32, bin order of FFTW (with half_band_shift: DC in bin n/2).  Asynchronous on `stream`. */
int  sdrhip_spectrum_run_device(sdrhip_spectrum *s, void *stream, const void *d_in, int64_t n_samples, int64_t hop,
                                int rows, float *d_out);
/* HOST vectors, synchronous (like sdrhip_fft_run) */
int  sdrhip_spectrum_run(sdrhip_spectrum *s, const void *in, int64_t n_samples, int64_t hop, int rows, float *out);
int  sdrhip_spectrum_set_route(sdrhip_spectrum *s, int route);   /* 0 = auto, 1 = the one-kernel route, 2 = hipFFT route */
long long sdrhip_debug_spectrum_fused_launches(void);            /* process-wide, for tests that assert the route */
/* process-wide: hipFFT transforms (one per chunk of rows that fits the scratch buffer) the operator has issued, from
 * sdrhip_spectrum_run_device and sdrhip_spectrum_reduce_run_device alike: tests of the chunking assert that it happened */
long long sdrhip_debug_spectrum_hipfft_batches(void);
/* Input addresses: u8 input may start at any address.  float32 input must be 4-byte aligned, else SDRHIP_ERR_ARG before any launch
 * with nothing written (an 8-byte aligned base is read with one load per sample, any other with two); int16 as stated at
 * SDRHIP_IQ_I16.  No byte outside the n_samples samples of d_in is read.
 * Non-finite float32 input (u8 and int16 cannot produce any): a NaN or an Inf in a sample makes EVERY bin of every row that holds
 * the sample non-finite -- NaN in every bin for a NaN sample, also where the window is 0 there (0 * NaN is NaN) -- and leaves every
 * other row's bits alone.  In the reducing form below such a row poisons its output row in every reduce and unit: all bins NaN for a
 * NaN sample, all bins non-finite for an Inf; the max hold does not drop the row and the dB floor does not hide it.  Which NaN
 * (sign, payload) is unspecified.  Both routes behave so. */

/* The operator's rows reduced on the device: output row R is made of the `group` consecutive input rows R*group .. R*group + group - 1
 * (input row r = samples [r*hop, r*hop + n), as above), which never reach memory.  With m_r[k] = scale * |X_r[k]|, exactly the double
 * sdrhip_spectrum_run_device rounds to float32, all arithmetic in double, no FMA:
 *     MEAN_POWER v = (sum of m^2) / group;  MEAN_MAGNITUDE v = (sum of m) / group;  MAX_MAGNITUDE v = max m;
 *     LINEAR out = (float)v;  DB out = (float)max(floor_db, c log10 v), c = 10 for MEAN_POWER and 20 otherwise (v = 0 gives floor_db).
 * SUMMATION ORDER (part of the definition): the group is cut into chunks of 32 consecutive input rows (the last may be shorter); each
 * chunk is summed in ascending row order starting from 0.0; the chunk sums are then added in ascending order starting from 0.0.
 * Needs rows_out >= 1, group >= 1, hop >= 1, (rows_out*group - 1)*hop + n <= n_samples, rows_out*group within int, reduce and unit
 * in range and a finite floor_db; otherwise SDRHIP_ERR_ARG, no launch, nothing written.  Asynchronous on `stream`.
 * On the one-kernel route an output row's bits depend on its own (group-1)*hop + n samples, group, reduce and unit alone: not on
 * rows_out, its place in the batch, the split mode or the grid; between the two routes the tolerance contract holds.  Groups of more
 * than 32 rows, and the hipFFT route, go through a bounded scratch buffer of the object (doubles per output bin, not per input row).
 * Split: with few output rows and a long group the chunks of a group are spread over the chip and added up by a second kernel, in
 * the order above (the same bits); `auto` does so when the output rows alone would leave compute units idle. */
#define SDRHIP_REDUCE_MEAN_POWER     0   /* Welch: mean over the group of m^2 */
#define SDRHIP_REDUCE_MEAN_MAGNITUDE 1   /* mean over the group of m          */
#define SDRHIP_REDUCE_MAX_MAGNITUDE  2   /* max hold: max over the group of m */
#define SDRHIP_UNIT_LINEAR 0
#define SDRHIP_UNIT_DB     1             /* 10 log10 v (power) / 20 log10 v (magnitudes), never below floor_db */
int  sdrhip_spectrum_reduce_run_device(sdrhip_spectrum *s, void *stream, const void *d_in, int64_t n_samples, int64_t hop,
                                       int rows_out, int group, int reduce, int unit, double floor_db, float *d_out /* rows_out x n */);
/* HOST vectors, synchronous */
int  sdrhip_spectrum_reduce_run(sdrhip_spectrum *s, const void *in, int64_t n_samples, int64_t hop, int rows_out, int group,
                                int reduce, int unit, double floor_db, float *out);
int  sdrhip_spectrum_set_reduce_split(sdrhip_spectrum *s, int mode);   /* 0 = auto, 1 = never, 2 = always (groups of more than 32 rows) */
/* process-wide: reduce calls that spread a group over workgroups.  Every reduce call on the one-kernel route also counts once in
 * sdrhip_debug_spectrum_fused_launches. */
long long sdrhip_debug_spectrum_reduce_split_launches(void);
/* process-wide: launches of the layered kernel, one per (slice of output rows, slice of chunks) that the bounded scratch buffer cuts
 * a reduce call of more than 32 rows per group into: tests of the slicing assert that it happened */
long long sdrhip_debug_spectrum_reduce_layer_launches(void);

/* ------------------------------------------------------------------------ */
/* (3) Pipe operators on host blocks                                        */
/* ------------------------------------------------------------------------ */
typedef struct sdrhip_pipe sdrhip_pipe;
/* The constructors take ownership of nothing: the descriptor must outlive the pipe. */
int sdrhip_pipe_fir_filter(sdrhip_pipe **p, const sdrhip_filter *f, int block_size_out);          /* firFilter   */
int sdrhip_pipe_fir_decimator(sdrhip_pipe **p, const sdrhip_decimator *d, int block_size_out);    /* firDecimator */
int sdrhip_pipe_fir_resampler(sdrhip_pipe **p, const sdrhip_resampler *r, int block_size_out);    /* firResampler */
int sdrhip_pipe_fm_demod(sdrhip_pipe **p);                                                         /* fmDemod      */
/* amDemod (sdrhip_am_demod_run) on host blocks: complex blocks in, float blocks of the same length out, like
 * sdrhip_pipe_fm_demod, and with its submission rule: staged blocks go out as one run, read and written in place over PCIe up
 * to 512 KiB of input, through the copy engines beyond.  Nothing is carried from block to block, so save / restore carry
 * only the output not yet popped; restore refuses (SDRHIP_ERR_ARG, the pipe unchanged) a state of another kind -- an fmDemod
 * pipe's included -- and a truncated one.  set_adaptive, flush, poll and pop as for the other map pipes; set_coalesce,
 * input_buffer and pop_rows are the filter-like pipes' and refuse a map pipe. */
int sdrhip_pipe_am_demod(sdrhip_pipe **p);                                       /* P.map (VG.map magnitude) */
int sdrhip_pipe_dc_blocker(sdrhip_pipe **p);                                     /* dcBlockingFilter, Filter.hs:730-739 */
/* complex blocks in, complex blocks out at the length they came in; the state starts at 1 and is carried across blocks on the
 * device (sdrhip_agc_run).  save / restore carry the state; mu and reference are the constructor's, not part of it. */
int sdrhip_pipe_agc(sdrhip_pipe **p, float mu, float reference);                 /* agcPipe, Util.hs:344-348 */
/* De-emphasis (sdrhip_deemph_run) on host blocks: float blocks in, float blocks out at the length they came in, a map stage like
 * sdrhip_pipe_dc_blocker: staged blocks go out as ONE run over all of them, from and to the state on the device (one float, starting
 * at 0), never read in place.  alpha as sdrhip_deemph_run takes it (SDRHIP_ERR_ARG otherwise, *p NULL).  It is a second form of the
 * one-pole map kind, not a kind of its own: a saved state holds the dcBlocker's kind number, the state in the first of its four
 * state floats and alpha in the third (a dcBlocker's third is 0, as it always was).  Restore refuses, leaving the pipe fresh, a
 * dcBlocker state into a de-emphasis pipe, the reverse, and a de-emphasis state of another alpha (compared as bits). */
int sdrhip_pipe_deemph(sdrhip_pipe **p, float alpha);
/* `P.map (VG.zipWith (*) osc) >-> firDecimator deci n` with osc indexed by the stream position: cfloat blocks in, blocks of exactly
 * block_size_out decimated samples out.  Push, pop, coalesce, adaptive, input_buffer, save and restore behave as for
 * sdrhip_pipe_fir_decimator; the stream position that selects the oscillator phase is part of the saved state (the table and
 * the taps are the descriptor's, not part of it).  The tuner must outlive the pipe. */
int sdrhip_pipe_tuner(sdrhip_pipe **p, const sdrhip_tuner *t, int block_size_out);
/* The tuner bank on host blocks: cfloat blocks (input_u8 = 0) or interleaved u8 IQ blocks (input_u8 = 1) in, every channel's blocks
 * of exactly block_size_out decimated samples out, in lockstep.
 * Definition: channel j's blocks equal, bit for bit, those of a sdrhip_pipe_tuner over a sdrhip_tuner of the bank's arguments with
 * table j, of the same block_size_out, fed the same blocks at the same boundaries -- for a u8 pipe fed (u - 128) * (1 / 128) as
 * float32, which is exact.  This holds whatever the push sizes, coalescing, adaptive submission or route; nothing new is argued.
 * Rows: sdrhip_pipe_rows is the bank's channel count (1 for every other pipe).  The counts push / flush / poll / restore return are
 * blocks PER CHANNEL.  sdrhip_pipe_pop_rows writes up to max_blocks blocks of every row, row j's nb * block_size_out elements to
 * out + j * row_stride floats, and returns nb; row_stride < max_blocks * block_size_out * (floats per element) is SDRHIP_ERR_ARG
 * with nothing written.  It serves every filter / decimator / resampler / tuner pipe (one row).  sdrhip_pipe_pop keeps its meaning
 * on one row (a one-channel bank included); on more rows it is SDRHIP_ERR_ARG and pops nothing.
 * Input type: a u8 pipe takes sdrhip_pipe_push_u8 / sdrhip_pipe_input_buffer_u8 (n_samples (I, Q) byte pairs), every other pipe
 * sdrhip_pipe_push / sdrhip_pipe_input_buffer; the wrong call is SDRHIP_ERR_ARG (NULL) with nothing staged.  u8 blocks cross the
 * link as 2 bytes per sample and are converted in the kernels' loaders.
 * Submission: equal-sized blocks go out as ONE sdrhip_tuner_bank_run over [carried tail | staged] with the block size as seam_block
 * (its route rule decides banked or channel by channel); a block of another size as one all-Cross launch for all channels over the
 * outputs that straddle the boundary (sdrhip_debug_tuner_bank_cross_launches) and one run with seam_block 0 for the rest.  A pipe of
 * more than one row never reads its input in place over PCIe -- K channels would fetch the same tile over the link K times: up to
 * 512 KiB a submission is one copy on its slot's stream and the launch behind it, beyond that the copy engines; the copy lands so
 * that the launch's first window is 16-byte aligned, whatever the block sizes were.  One row follows sdrhip_pipe_tuner's rule.
 * Coalesce, adaptive (its byte cap counts input bytes: 2 per u8 sample), flush, poll and destroy as for sdrhip_pipe_tuner.
 * Save / restore: a pipe of more than one row or of u8 input writes a state version of its own -- row count, input type, stream
 * position, the history in the input's own type and every row's output not yet popped; restore refuses (SDRHIP_ERR_ARG, the pipe
 * unchanged) a state of another row count, input type, block_size_out, factor or tap count, and a truncated one.
 * Create: SDRHIP_ERR_ARG (and *p = NULL) before any device work for a null argument, block_size_out <= 0 and input_u8 outside 0 / 1.
 * The bank must outlive the pipe. */
int sdrhip_pipe_tuner_bank(sdrhip_pipe **p, const sdrhip_tuner_bank *b, int block_size_out, int input_u8);
int sdrhip_pipe_rows(const sdrhip_pipe *p);
int sdrhip_pipe_push_u8(sdrhip_pipe *p, const uint8_t *iq, int n_samples);
uint8_t *sdrhip_pipe_input_buffer_u8(sdrhip_pipe *p, int n_samples);
/* The tuner bank on host blocks of interleaved int16 IQ (4 bytes per sample from the staging buffer to the kernels' loaders).
 * Definition: sdrhip_pipe_tuner_bank's, with c(s) = (float)s * 2^-11 in place of (u - 128) * (1 / 128): channel j's blocks are those
 * of a one-row sdrhip_pipe_tuner with table j fed the same blocks as c(.) floats at the same boundaries.  Such a pipe takes
 * sdrhip_pipe_push_i16 / sdrhip_pipe_input_buffer_i16 (n_samples (I, Q) int16 pairs); the wrong call for a pipe's input type -- any
 * of the three -- is SDRHIP_ERR_ARG (NULL) with nothing staged.  The carried tail starts at a multiple of 4 samples; rows, submission,
 * coalesce, adaptive (4 bytes per sample) and flush as above.  Saved states are version 2 with input type 2 and the history as
 * int16; restore refuses an int16 state on a cfloat or u8 pipe and the reverse, the pipe unchanged.
 * Create: SDRHIP_ERR_ARG (and *p = NULL) before any device work for a null argument and block_size_out <= 0. */
int sdrhip_pipe_tuner_bank_i16(sdrhip_pipe **p, const sdrhip_tuner_bank *b, int block_size_out);

/* The AM bank (sdrhip_am_bank_*) on host blocks: cfloat (input_type 0, sdrhip_pipe_push / _input_buffer), u8 IQ (1, _push_u8 /
 * _input_buffer_u8) or int16 IQ (2, _push_i16 / _input_buffer_i16) blocks in, every channel's audio out in blocks of exactly
 * block_size_out FLOATS through sdrhip_pipe_pop_rows / sdrhip_pipe_rows (sdrhip_pipe_pop with one channel).
 * Definition: channel j's blocks are sdrhip_pipe_tuner_bank's blocks of the same pushes, put through `magnitude` (amDemod) and, when
 * the bank was created with dc_block = 1, through dcBlocker from (0, 0) (`func 0 0`, Filter.hs:731) over the whole stream: both are
 * independent of the block sizes.  Bit for bit, for every sequence of block sizes, coalesced or adaptive.
 * Machinery: sdrhip_pipe_tuner_bank's, with one float per output -- the [carried tail | staged] copy, the 16-byte alignment of the
 * first window in device memory, equal blocks as ONE envelope run with the block size as seam_block (one envelope tile launch,
 * sdrhip_debug_am_bank_launches), a block of another size as the all-Cross envelope launch over the outputs that straddle the
 * boundary (sdrhip_debug_am_bank_cross_launches) plus one run with seam_block 0.  The envelope launches are the AM bank's fused route
 * wherever it fits, whatever the bank's route setting and auto rule (those belong to sdrhip_am_bank_run); a bank of another order or
 * factor goes through the tuner bank and amDemod's rows form.  The input is NEVER read in place, whatever the row count (a stated choice:
 * the FM bank stream's sweep found no in-place region): up to 512 KiB a submission is one copy and its launches on one stream.
 * dcBlocker runs behind the envelope on the device: the K state pairs live in device memory, zero at create, and there is no host
 * synchronisation between pushes.  ORDERING: dcBlocker makes consecutive submissions depend on each other, so every launch of a pipe
 * with dc_block goes to ONE compute stream (the engine's first) and is ordered behind the previous submission's by that stream; without
 * dc_block the submissions stay as independent as sdrhip_pipe_tuner_bank's (a stream per slot).
 * sdrhip_pipe_set_coalesce / _set_adaptive, sdrhip_pipe_flush / _poll as for sdrhip_pipe_tuner_bank; the push call of another input
 * type is SDRHIP_ERR_ARG.  Save / restore: the rows state of sdrhip_pipe_tuner_bank plus dc_block and the 2 K dcBlocker floats (save
 * flushes, then reads them back, as the dcBlocker Pipe's save); restore refuses another kind, row count, input type, block_size_out,
 * factor, tap count or dc_block and a truncated state, with the pipe unchanged.  The kind number is a new one at the end: states of
 * every other kind keep their bytes.  SDRHIP_ERR_ARG (and *p = NULL) before any device work for a null bank, block_size_out <= 0 and
 * an input_type outside 0 .. 2.  The AM bank (and its tuner bank) is borrowed and must outlive the pipe. */
int sdrhip_pipe_am_bank(sdrhip_pipe **p, const sdrhip_am_bank *b, int block_size_out, int input_type);
/* The narrow-band FM bank (sdrhip_nfm_bank_*) on host blocks: cfloat (input_type 0), u8 IQ (1) or int16 IQ (2) blocks in through the
 * push and input_buffer calls of that type, every channel's demodulated blocks of exactly block_size_out FLOATS out through
 * sdrhip_pipe_pop_rows / sdrhip_pipe_rows (sdrhip_pipe_pop with one channel).
 * Definition: channel j's blocks are sdrhip_pipe_tuner_bank's blocks of the same pushes put through the reference's fmDemod Pipe
 * (Demod.hs:40-46), started from (0, 0); fmDemod carries only the last sample, so block boundaries do not matter to it.  Bit for bit,
 * for every sequence of block sizes, coalesced or adaptive.
 * Machinery: sdrhip_pipe_am_bank's -- the [carried tail | staged] copy, the 16-byte alignment of the first window in device memory,
 * equal blocks as ONE fmDemod-form tile launch with the block size as seam_block (sdrhip_debug_nfm_bank_launches), a block of another
 * size as one all-Cross fmDemod-form launch over the outputs that straddle the boundary (sdrhip_debug_nfm_bank_cross_launches) plus
 * one tile launch with seam_block 0.  The launches are the bank's fused route wherever it fits, whatever the bank's route setting and
 * auto rule; a bank of another order or factor goes through the tuner bank and fmDemod's rows form.  The input is never read in place.
 * STATE: two arrays of K (re, im) pairs live in device memory, zero at create; every launch reads one and writes the other, and they
 * are swapped after every launch.  There is no host synchronisation between pushes.  ORDERING: consecutive submissions depend on
 * each other through that state, so every launch of this pipe goes to ONE compute stream (the engine's first).
 * sdrhip_pipe_set_coalesce / _set_adaptive, sdrhip_pipe_flush / _poll as for sdrhip_pipe_tuner_bank; the push call of another input
 * type is SDRHIP_ERR_ARG.  Save / restore: the rows state of sdrhip_pipe_tuner_bank plus the 2 K state floats (save flushes, then
 * reads them back); restore refuses another kind, row count, input type, block_size_out, factor, tap count and a truncated state,
 * with the pipe unchanged.  The kind number is a new one at the end (11): states of every other kind keep their bytes.
 * SDRHIP_ERR_ARG (and *p = NULL) before any device work for a null bank, block_size_out <= 0 and an input_type outside 0 .. 2.  The
 * bank (and its tuner bank) is borrowed and must outlive the pipe. */
int sdrhip_pipe_nfm_bank(sdrhip_pipe **p, const sdrhip_nfm_bank *b, int block_size_out, int input_type);
/* The two banks with their audio stages, on host blocks: IQ blocks in (input_type and the push / input_buffer calls as above), every
 * channel's AUDIO out in blocks of exactly `block` floats -- the block the tail was created with, at least 1 -- through
 * sdrhip_pipe_pop_rows / sdrhip_pipe_rows (sdrhip_pipe_pop with one channel), every row in lockstep.
 * Definition: channel j's blocks are those of  sdrhip_pipe_am_bank / sdrhip_pipe_nfm_bank with block_size_out = block
 * >-> firResampler(block) >-> firFilter(block) >-> (* gain)  over the same pushes, bit for bit, for every sequence of block sizes,
 * coalesced or adaptive.
 * Per submission: the bank part is the bank Pipe's -- the same launches, states and alignment, everything on ONE compute stream (the
 * engine's first) -- but its demodulated rows stay on the device, behind the elements carried from earlier submissions; then ONE
 * sdrhip_audio_tail_run_rows computes the audio outputs that became ready (sdrhip_audio_tail_ready of the demodulated count so
 * far) into the result, on the tail's route (auto: sdrhip_audio_tail_set_route); then the elements from the next audio output's
 * first input on (at most sdrhip_audio_tail_max_halo per row) are copied to the front of a second rows buffer by a 2-D device copy.
 * A submission that completes no audio output runs the bank part and no tail launch.  No host synchronisation between pushes once
 * the rows buffers and the tail's workspace have the size of the largest push.
 * Save / restore: the bank Pipe's state for that kind, the audio position, the tail's shape and the carried rows read back from
 * the device (save flushes).  Restore refuses another kind, row count, input type, block, factor, tap count, dc_block, resampler
 * ratio, other tail tap counts and a truncated state, with the pipe unchanged.  The kind numbers are new ones at the end (12, 13):
 * states of every other kind keep their bytes.  SDRHIP_ERR_ARG (and *p = NULL) before any device work for a null bank, a null tail,
 * a tail of block 0 and an input_type outside 0 .. 2.  The bank and the tail are borrowed and must outlive the pipe. */
int sdrhip_pipe_am_bank_audio(sdrhip_pipe **p, const sdrhip_am_bank *b, const sdrhip_audio_tail *tail, int input_type);
int sdrhip_pipe_nfm_bank_audio(sdrhip_pipe **p, const sdrhip_nfm_bank *b, const sdrhip_audio_tail *tail, int input_type);
/* The narrow-channel bank (sdrhip_narrow_bank_*) on host blocks:
 *     firDecimator deci1 block_mid >-> firDecimator deci2 block_size_out >-> P.map (magnitude | fmDemod) [>-> dcBlockingFilter]
 * for the K channels, cfloat (input_type 0), u8 IQ (1) or int16 IQ (2) blocks in, blocks of block_size_out floats per channel out
 * through sdrhip_pipe_pop_rows / _pop.  The narrow bank -- and through it the tuner bank and the second decimator -- is BORROWED.
 * The bank part of a submission is the tuner bank Pipe's, unchanged (the uniform route and the ragged route: one all-Cross launch plus
 * one banked launch), but writes its complex rows behind the carried history of a device rows buffer: the mechanism of the audio
 * Pipes with complex elements.  ONE narrow run then computes the stage-2 outputs that became ready -- those of the WHOLE blocks of
 * block_mid stage-1 outputs so far: stage 2 only ever sees blocks of exactly block_mid, whatever the push sizes were -- with
 * seam_block2 = block_mid into the result chunk: the fused launch (route 1 of sdrhip_narrow_bank_run) wherever it fits, else the
 * composed calls, whatever the bank's route setting and auto rule; a 2-D device copy carries the rows' unread tail to the front of a
 * second buffer.  A submission that completes no stage-2 output runs the bank part only.  Every launch goes to ONE compute stream.
 * Save / restore: the bank Pipe's state plus the stage-2 position, block_mid, the second decimator's factor and prepared length, the
 * form, dc_block, fmDemod's pairs or dcBlocker's state, and the carried complex rows; restore refuses every mismatch of these.  Kind
 * number 14; the states of all other kinds keep their bytes.  SDRHIP_ERR_ARG (and *p = NULL), before any device work: a null pointer
 * or bank, block_size_out < 1, an input_type outside 0 .. 2, block_mid < numCoeffs + factor of the second decimator (the reference's
 * `assert "decimate 1"`: after a crossover a block still holds one whole filter). */
int sdrhip_pipe_narrow_bank(sdrhip_pipe **p, const sdrhip_narrow_bank *b, int block_mid, int block_size_out, int input_type);
/* The narrow-channel bank with the audio stages behind it, on host blocks:
 *     firDecimator deci1 block_mid >-> firDecimator deci2 block >-> P.map (magnitude | fmDemod) [>-> dcBlockingFilter]
 *     >-> firResampler(block) >-> firFilter(block) >-> (* gain)
 * for the K channels, `block` the block the tail was created with (at least 1); every channel's AUDIO out in blocks of exactly
 * `block` floats through sdrhip_pipe_pop_rows / _pop.  Definition: channel j's blocks are those of sdrhip_pipe_narrow_bank with
 * block_size_out = block, popped and pushed through sdrhip_pipe_fir_resampler(block) and sdrhip_pipe_fir_filter(block) and scaled by
 * the gain, bit for bit, for every sequence of push sizes, coalesced or adaptive.
 * Per submission: the bank part and the narrow run are the narrow Pipe's, but stage 2 writes its REAL rows behind the carried history
 * of a second device rows buffer instead of into the result; ONE sdrhip_audio_tail_run_rows then computes the audio outputs that
 * became ready -- sdrhip_audio_tail_ready of the stage-2 outputs so far -- into the result on the tail's route (route 0: the general
 * fused kernel where sdrhip_audio_tail_set_general's rule or mode 1 says so); then both carries step.  A submission that completes no
 * stage-2 output runs the bank part only; one that completes stage-2 outputs but no audio output runs no tail launch.  Every launch
 * goes to ONE compute stream.
 * Save / restore: the kind number stays 14.  The narrow record's last field (always 0 so far) is has_tail = 1, and an audio record
 * follows it: the audio position, sdrhip_audio_tail_shape, and the carried real stage-2 rows.  A plain narrow pipe's state keeps every
 * byte.  Restore refuses, with the pipe left fresh: a tailed state on a plain narrow pipe and the reverse, another tail shape, every
 * mismatch the narrow record refuses, and a truncated state.  SDRHIP_ERR_ARG (and *p = NULL), before any device work: a null
 * pointer, bank or tail, a tail of block 0, an input_type outside 0 .. 2, block_mid < numCoeffs + factor of the second decimator.
 * The bank and the tail are borrowed and must outlive the pipe. */
int sdrhip_pipe_narrow_bank_audio(sdrhip_pipe **p, const sdrhip_narrow_bank *b, const sdrhip_audio_tail *tail, int block_mid, int input_type);
int sdrhip_pipe_push_i16(sdrhip_pipe *p, const int16_t *iq, int n_samples);
int16_t *sdrhip_pipe_input_buffer_i16(sdrhip_pipe *p, int n_samples);

/* The waterfall on host blocks: raw IQ blocks of ANY size >= 1 sample in, spectrum rows out.
 * Input: the type of the spectrum object -- a cfloat object's pipe takes sdrhip_pipe_push / _input_buffer (n complex samples), a u8
 * one _push_u8 / _input_buffer_u8, an int16 one _push_i16 / _input_buffer_i16 (n_samples (I, Q) pairs); the wrong call for the pipe's
 * type is SDRHIP_ERR_ARG (NULL) with nothing staged.
 * Output: blocks of exactly n floats, one output row each.  sdrhip_pipe_pop returns n, or 0 if no row is ready; a capacity below n is
 * SDRHIP_ERR_ARG with nothing written and nothing popped.  sdrhip_pipe_pop_rows serves it as a one-row pipe with block_size_out = n;
 * sdrhip_pipe_rows is 1.  The counts push / flush / poll / restore return are output rows.
 * Definition: with S the concatenation of every sample pushed so far, output row R exists as soon as
 * (R * group + group - 1) * hop + n <= |S| and is row R of
 *     sdrhip_spectrum_reduce_run_device(s, stream, S, |S|, hop, rows_out, group, reduce, unit, floor_db, out).
 * With group 1, MEAN_MAGNITUDE and LINEAR that is sdrhip_spectrum_run_device's row; with hop = n it is the reference's waterfall pipe
 * (one block of n samples, one row).  On the one-kernel route the rows equal that one call's BIT FOR BIT, for every sequence of push
 * sizes, coalesced or adaptive, and every group length (a row's bits depend on its own samples, group, reduce and unit alone); on the
 * hipFFT route the operator's tolerance contract holds.  Nothing new is argued.
 * Machinery: the host keeps the samples from the first row not yet produced onward, in the input's own type (the engine's
 * [carried tail | staged]).  A push that completes no output row launches nothing.  A submission that completes r >= 1 rows is ONE
 * reduce run over [tail | staged] with rows_out = r (one count of sdrhip_debug_spectrum_fused_launches on the one-kernel route).  The
 * next tail starts at stream sample rows_done * group * hop; with hop > n that can lie beyond what has been pushed, and the samples in
 * between are dropped on arrival, never staged.  The stream position is 64-bit.
 * Submission: the input is NEVER read in place over PCIe (with hop < n every sample is read n / hop times): up to 512 KiB a submission
 * is one copy on its slot's stream and the launch behind it, beyond that the copy engines (a stated choice, not a measured one).
 * ORDERING: the spectrum object has one scratch buffer.  A submission that does not touch it (one-kernel route, group <= 32) keeps a
 * stream per slot; every submission that does (hipFFT route, groups of more than 32 rows, split or not) goes to ONE compute stream
 * (the engine's first) and is ordered behind its predecessor by it.  Up to four submissions are in flight.
 * MAY BLOCK THE HOST: a push / flush that reopens a slot waits for that slot's previous submission (as every pipe); on the hipFFT route
 * a submission whose batch of rows needs a transform plan the object has not kept waits for the object's last run, and one that needs
 * a larger work buffer than any before waits for the device (the rules of sdrhip_spectrum_reduce_run_device, unchanged).  Every other
 * push returns without waiting for the GPU.
 * Borrowing: the pipe borrows the spectrum object EXCLUSIVELY: the object must outlive the pipe, its route and split settings are read
 * at every submission, and a direct sdrhip_spectrum_*run* call on it while the pipe holds submissions in flight (before a flush) is
 * the caller's error.
 * sdrhip_pipe_set_coalesce(N > 1): a submission waits for N complete rows; sdrhip_pipe_set_adaptive(M): rows pile up (up to M rows or
 * 4 MiB of input) while the slot a submission would move on to is still running; flush submits every complete row and drains; poll
 * and destroy as for the filter-like pipes.  Results never depend on them.
 * Save / restore: a state version and kind of its own (the kind number is a new one at the end; states of every other kind keep their
 * bytes): uint32 magic, version (3); int32 kind, n, input type (0 cfloat, 1 u8, 2 int16), group, reduce, unit; int64 hop; double
 * floor_db; int64 stream position, rows produced, skip count, tail samples, pending floats; then the tail in the input's type and the
 * rows not yet popped.  Restore refuses (SDRHIP_ERR_ARG, the pipe unchanged) a state of another kind, a difference in n, input type,
 * hop, group, reduce, unit or floor_db, and a truncated or inconsistent state.
 * Create: SDRHIP_ERR_ARG (and *p = NULL) before any device work for a null argument, hop < 1, group < 1, reduce or unit out of range,
 * a non-finite floor_db, and a carried tail that could exceed 4 MiB: ((group - 1) * hop + n - 1) * (bytes per sample) > 4 MiB (the
 * engine's adaptive staging cap: a stated bound; carrying partial group sums on the device instead is out of scope). */
int sdrhip_pipe_spectrum(sdrhip_pipe **p, sdrhip_spectrum *s, int64_t hop, int group, int reduce, int unit, double floor_db);
int sdrhip_pipe_pop_rows(sdrhip_pipe *p, float *out, int64_t row_stride, int max_blocks);
/* Feed one upstream block (n elements: floats, or complex pairs for complex
 * stages).  Returns the number of complete output blocks now ready (>= 0) or a
 * negative error.  A block shorter than numCoeffs is the reference's
 * `assert "filter 1"` failure -> SDRHIP_ERR_ARG. */
int sdrhip_pipe_push(sdrhip_pipe *p, const float *block, int n);
/* Up to four submissions are in flight (SDRHIP_STREAM_SLOTS=2..4), so results lag up to three pushes behind: flush waits
 * for the in-flight blocks and returns the number of complete output blocks ready. */
/* Throughput knobs of the filter / decimator / resampler pipes (results never depend on them):
 *  - set_coalesce(blocks): equal-sized pushes are staged in the pinned buffer and submitted `blocks` at a
 *    time (one upload, one run over the batch with its interior seams, one download); a push of another
 *    size ends the uniform run.  0 / 1 = every push on its own.  blocks > 1 takes precedence over adaptive submission
 *    (exactly `blocks` per submission, whatever the GPU is doing).
 *  - set_adaptive(max_blocks): the same, decided by the GPU: a push is submitted at once while the slot its submission would
 *    move on to is free, and staged behind the earlier ones while that slot is still running (up to max_blocks, and never more
 *    than 4 MiB of staged input (SDRHIP_ADAPTIVE_BYTES; batches past 512 KiB go through the copy engines instead of being read
 *    in place over PCIe); a source slower than the GPU sees every push go out immediately, a faster
 *    one sees fewer, larger launches.  Which push returns which block then depends on timing.  0 = off.
 *  - input_buffer(n): the pinned staging memory the next push of n elements will be uploaded from; fill it
 *    and push that pointer to skip the host-side copy. */
int sdrhip_pipe_set_coalesce(sdrhip_pipe *p, int blocks);
int sdrhip_pipe_set_adaptive(sdrhip_pipe *p, int max_blocks);
float *sdrhip_pipe_input_buffer(sdrhip_pipe *p, int n);
int sdrhip_pipe_flush(sdrhip_pipe *p);
/* output blocks ready to pop, after collecting (without waiting) every in-flight submission the GPU has finished */
int sdrhip_pipe_poll(sdrhip_pipe *p);
/* Pop one ready block into out (capacity in elements); returns its length, 0 if none. */
int sdrhip_pipe_pop(sdrhip_pipe *p, float *out, int capacity);
/* Checkpoint / resume, as sdrhip_fm_stream_save / _restore: save drains the pipe (like flush) and writes its state -- position,
 * the last few input elements, the carried fmDemod sample / dcBlocker pair, the output not yet popped; restore loads it into a
 * freshly created pipe of the same kind over a descriptor of the same taps; returns the blocks ready to pop. */
/* state_bytes drains the pipe (like flush) and returns the exact size the save that follows needs (0 = the drain failed). */
size_t sdrhip_pipe_state_bytes(sdrhip_pipe *p);   /* not const: it drains (submits, waits, moves results) */
int sdrhip_pipe_save(sdrhip_pipe *p, void *buf, size_t capacity, size_t *used);
int sdrhip_pipe_restore(sdrhip_pipe *p, const void *buf, size_t bytes);
void sdrhip_pipe_destroy(sdrhip_pipe *p);

#ifdef __cplusplus
}
#endif
#endif /* SDR_HIP_H */
