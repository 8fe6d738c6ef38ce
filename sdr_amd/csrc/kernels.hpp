// kernels.hpp -- host-callable launchers of the gfx950 kernels (internal header).
//
// Every launcher is asynchronous on `stream` and works on DEVICE pointers.  The
// arithmetic contract (summation orders, no FMA) is documented per kernel in
// kernels_generic.hip / kernels_fast.hip; the file is compiled with
// -ffp-contract=off, which the parity of every result depends on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrhip {

// Which reference variant's summation order is reproduced.
//  real data:    lanes 1 (scalar), 4 (SSE), 8 (AVX)            common.h:34-72
//  complex data: CO_SEQ   scalar                                common.h:95-106
//                CO_L2/L4 "RC":  duplicated taps, 2/4 complex lanes  (decimate.c:84-113)
//                CO_X2/X4 "RC2": plain taps, 4/8 complex partials folded (common.h:108-155)
enum ComplexOrder { CO_SEQ = 0, CO_L2 = 1, CO_L4 = 2, CO_X2 = 3, CO_X4 = 4 };

// Stream geometry of one launch (see include/sdr_hip.h "Stream semantics").
struct Geom {
    int64_t in_base;   // global index of in[0]
    int64_t k_begin;   // global index of out[0]
    int     count;     // outputs in this launch
    int     I;         // interpolation (1 for filter / decimator)
    int     D;         // decimation
    int     Lp;        // Pipe-visible (padded) length in upsampled units
    int64_t seamBI;    // seam_block * I; 0 = contiguous (all One); < 0 = every output Cross
    int64_t outB = 0;  // the Pipe's output block size (0 = unbounded): see late_output_is_one below
};

// Does the reference's Pipe enter its crossover (sequential) code at the buffer boundary `edge` (upsampled units, a
// multiple of seamBI)?  m* = the first output whose window no longer fits the buffer ending at `edge`; the Pipe crosses
// over iff m*'s first input sample, ceil(m* D / I), still lies in that buffer -- and then computes EVERY output whose
// virtual start m D is before the edge sequentially (firResampler: `outputsComputable`, Filter.hs:712-716).  Otherwise
// (`VG.length bufIn' == 0 -> simple next`, Filter.hs:707-709; only possible when I > 1) m* is simply the first SIMD
// output of the next buffer and the seam has no sequential outputs at all.  For I == 1 both tests coincide.
__host__ __device__ inline bool seam_has_crossover(int64_t edge, int I, int D, int Lp)
{
    if (I == 1) return true;
    const int64_t m_star = edge >= Lp ? (edge - Lp) / D + 1 : 0;
    const int64_t first_in = (m_star * D + I - 1) / I;
    return first_in * I < edge;
}

// Inside a crossover the Pipe computes every output whose virtual start precedes the boundary -- but only as far as
// its OUTPUT block has room (`count = min outputsComputable (space bufferOut)`, Filter.hs:715); when it comes back with a
// fresh output block it re-decides by the first input sample (`inputUsed >= VG.length bufLast -> simple`, Filter.hs:722-724).
// So the one output whose virtual start lies in the last I-1 zero-stuffed positions before the boundary (first input
// already in the next buffer) is sequential -- unless it is the first output of an output block, in which case it is the
// next buffer's first SIMD output.  outB = the output block size (global output index m = 0 starts a block).
__host__ __device__ inline bool late_output_is_one(int64_t m, int64_t edge, int I, int D, int64_t outB)
{
    if (I == 1 || outB <= 0 || m % outB != 0) return false;
    const int64_t first_in = (m * D + I - 1) / I;
    return first_in * I >= edge;
}

// Is output m of a seamed stream computed in the reference's sequential ("Cross") order?  One when the window fits the buffer it
// starts in; else Cross -- unless the Pipe never crosses over at that boundary (seam_has_crossover), or the output is the late
// first One of an output block.
__host__ __device__ inline bool is_cross(const Geom& g, int64_t m)
{
    if (g.seamBI == 0) return false;
    if (g.seamBI < 0) return true;   // every output of this launch is a seam straddler
    const int64_t v = m * (int64_t)g.D;
    const int64_t edge = (v / g.seamBI + 1) * g.seamBI;
    if (v + g.Lp <= edge) return false;
    if (late_output_is_one(m, edge, g.I, g.D, g.outB)) return false;
    return seam_has_crossover(edge, g.I, g.D, g.Lp);
}

// The seams of one launch, as every tiled launcher's fix-up sees them: the multiples of seamBI strictly inside the launch's
// window range [k_begin D, (k_end - 1) D + Lp) are first * seamBI ... (first + nseams - 1) * seamBI, and the straddlers of a
// seam are among the last `per` outputs whose window starts before it.  nseams = 0: a contiguous stream, or no seam inside.
struct SeamSpan {
    int64_t first;
    int nseams;
    int per;           // candidate slots per seam: ceil((Lp - 1) / D)
};
inline SeamSpan seam_span(const Geom& g)
{
    SeamSpan sp = {0, 0, (g.Lp - 1 + g.D - 1) / g.D};
    if (g.seamBI <= 0 || g.count <= 0) return sp;
    const int64_t v_lo = g.k_begin * g.D, v_hi = (g.k_begin + g.count - 1) * g.D + g.Lp;
    sp.first = v_lo / g.seamBI + 1;                      // first boundary strictly above v_lo
    const int64_t last = (v_hi - 1) / g.seamBI;          // last boundary strictly below v_hi
    if (last >= sp.first) sp.nseams = (int)(last - sp.first + 1);
    return sp;
}
// Inputs (from d_in[0]) the caller of a launch guarantees: the first input of its last output and the `reach` inputs that output
// walks (a filter / decimator: Lp; a resampler: the nloop floats of a group row).  The LDS-staged fix-ups clamp their loads to it.
inline int64_t seam_in_avail(const Geom& g, int reach)
{
    const int64_t last_m = g.k_begin + g.count - 1;
    return (last_m * g.D + g.I - 1) / g.I - g.in_base + reach;
}
// kernels_crossfix.hip: the generic fix-up kernels (one thread per candidate slot, any D / Lp / I, global reads), compiled once.
// Filter / decimator seams: real or complex data (complex: cfloat or interleaved u8 IQ input), sequential over the g.Lp taps of
// d_cross_taps; gain for real data only.  Nothing is launched when sp.nseams == 0.
void launch_fir_crossfix(hipStream_t s, const Geom& g, const SeamSpan& sp, bool cplx, bool in_is_u8, const float* d_cross_taps,
                         const void* d_in, float* d_out, float gain = 1.0f, bool apply_gain = false);
// Resampler seams, real or complex data: stride I over the `ntaps` UNPADDED taps.
void launch_resample_crossfix(hipStream_t s, const Geom& g, const SeamSpan& sp, bool cplx, const float* d_plain_taps, int ntaps,
                              const float* d_in, float* d_out);

// Real data ------------------------------------------------------------------
// taps: `ntaps` floats (multiple of lanes).  sym: taps are the HALF filter.
// cross_taps: Lp floats used by the sequential "Cross" outputs (may be null when seamBI == 0).
void launch_fir_real(hipStream_t s, const Geom& g, int lanes, bool sym, const float* d_taps, int ntaps,
                     const float* d_cross_taps, const float* d_in, float* d_out);

// Complex data, real taps.  For CO_L2/CO_L4 d_taps holds 2*P interleaved
// (duplicated) floats and ntaps = 2P; otherwise P plain taps.  sym => half taps
// (only with CO_X2/CO_X4: the reference's SymmetricRC kernels).
void launch_fir_cplx(hipStream_t s, const Geom& g, ComplexOrder order, bool sym, const float* d_taps, int ntaps,
                     const float* d_cross_taps, const float* d_in, float* d_out);
// same with interleaved u8 IQ input (convert fused into the load)
void launch_fir_cplx_u8(hipStream_t s, const Geom& g, ComplexOrder order, const float* d_taps, int ntaps,
                        const float* d_cross_taps, const uint8_t* d_in, float* d_out);

// Polyphase resampler.  Output i of the launch uses group (group0 + i) % ngroups
// and starts at input  pos0 + (i / ngroups) * period + pre[i % ngroups]  (relative
// to d_in).  groups: ngroups rows of `row_stride` floats; the dot product runs
// over nloop floats (roundUp(num_coeffs, lanes)).
struct ResampTable {
    int ngroups;
    int group0;
    int64_t pos0;
    int period;       // inputs consumed by one full cycle of groups
    int pre[64];      // prefix of increments starting at group0
    int row_stride;
    int nloop;
    // for Cross outputs (seams) and the legacy sequential resampler: plain taps,
    // filter offset of each group, and force_seq = every output sequential
    int ntaps_plain;
    int fo[64];
    int force_seq;
    // more than 64 groups (the reference's C runs any count, resample.c:34-142): the per-group tables live in device memory
    // instead of the kernel arguments -- ext[0 .. ngroups] = prefix sums of the increments from group 0 (ext[ngroups] = period),
    // ext[ngroups + 1 + g] = filter offset of group g -- and pre[] / fo[] above are unused.  Generic kernels only.
    const int* ext = nullptr;
};
void launch_resample_real(hipStream_t s, const Geom& g, int lanes, const ResampTable& t, const float* d_groups,
                          const float* d_plain_taps, const float* d_in, float* d_out);
void launch_resample_cplx(hipStream_t s, const Geom& g, ComplexOrder order, const ResampTable& t,
                          const float* d_groups, const float* d_plain_taps, const float* d_in, float* d_out);

// The cut of a polyphase launch for the kernels that compute whole cycles (group 0 .. ngroups - 1 per thread): `lead` outputs
// before the first group-0 output, `ncycles` whole cycles, `tail` outputs after them; the first cycle starts `skip` inputs
// behind t.pos0.  pre[]: ResampTable::pre (prefix from group0); increments: per group, from group 0.
struct CycleSplit {
    int lead, ncycles, tail;
    int done;          // outputs in front of the tail
    int64_t skip;
};
inline CycleSplit cycle_split(int ngroups, int group0, int count, const int* pre, const int* increments)
{
    CycleSplit c = {};
    c.lead = (ngroups - group0) % ngroups;
    if (c.lead > count) c.lead = count;
    c.ncycles = (count - c.lead) / ngroups;
    c.done = c.lead + ngroups * c.ncycles;
    c.tail = count - c.done;
    c.skip = c.lead > 0 ? pre[c.lead - 1] + increments[(group0 + c.lead - 1) % ngroups] : 0;
    return c;
}
// kernels_generic.hip: the lead-in and tail outputs of such a launch by the generic kernels, every output as One (the caller
// fixes its seams up afterwards); lanes for real data, corder for complex.
void launch_resample_lead_tail(hipStream_t s, const Geom& g, const CycleSplit& c, bool cplx, int lanes, ComplexOrder corder,
                               const ResampTable& t, const int* increments, const float* d_groups, const float* d_plain_taps,
                               const float* d_in, float* d_out);

// Element-wise ----------------------------------------------------------------
void launch_convert_u8(hipStream_t s, const uint8_t* d_in, float* d_out, int64_t n);
void launch_convert_i16(hipStream_t s, const int16_t* d_in, float* d_out, int64_t n);
void launch_convert_f32_to_i16_bladerf(hipStream_t s, const float* d_in, int16_t* d_out, int64_t n);
void launch_scale(hipStream_t s, float factor, const float* d_in, float* d_out, int64_t n);
// y[i] = phase(x[i] * conj(x[i-1])), i < count; x[-1] = d_in[-1] if has_prev else (last_re,last_im)
void launch_fm_demod(hipStream_t s, const float* d_in_iq, float* d_out, int64_t count, bool has_prev,
                     float last_re, float last_im);
// filter.c:152-161 (kernels_iir.hip: speculative chunks + verification, bit-exact with the sequential walk).
// d_final receives {finalSample, finalOutput}; d_ws (dc_blocker_workspace_bytes, may be null = sequential walk)
// starts with four u32 statistics {chunks left to the sequential settle, samples it rewrote, chunks recomputed in the
// parallel repair rounds, chunks of the launch (0 = the sequential walk)}; run_in <= 0 selects the default.  d_state, when
// given, holds {lastSample, lastOutput} on the device and overrides the two scalars (it may alias d_final: a Pipe chains
// its blocks that way).  num == 0 hands the state on to d_final.
struct DcPlan { int64_t C, W; int nchunks; };    // chunk length, run-in, chunks (0 = the sequential walk)
DcPlan dc_plan(int64_t num, int run_in);
size_t dc_blocker_workspace_bytes(int64_t num);
void launch_dc_blocker(hipStream_t s, int64_t num, float last_sample, float last_output, const float* d_in,
                       float* d_out, float* d_final, void* d_ws, int run_in, const float* d_state = nullptr);
// agc, Util.hs:325-342 (kernels_agc.hip: the same speculate / repair / settle scheme on interleaved complex samples,
// bit-exact with the sequential walk).  d_final receives the final state (one float); d_ws as for dcBlocker, with a fourth
// statistics word {chunks of the launch, 0 = the sequential walk}; run_in <= 0 selects the default, a function of mu.
// d_state, when given, holds the starting state on the device and overrides `state` (it may alias d_final).  num == 0
// hands the state on to d_final.
struct AgcPlan { int64_t C, W; int nchunks; };   // chunk length, run-in, chunks (0 = the sequential walk)
AgcPlan agc_plan(int64_t num, float mu, int run_in);
size_t agc_workspace_bytes(int64_t num);         // enough for any run_in
void launch_agc(hipStream_t s, int64_t num, float mu, float reference, float state, const float* d_in, float* d_out,
                float* d_final, void* d_ws, int run_in, const float* d_state = nullptr);

// Row forms (the "rows" sections of kernels_agc.hip, kernels_iir.hip, kernels_chain.hip): row r is d_in + r * in_stride ->
// d_out + r * out_stride, strides in floats.  States in and out live on the device (agc: rows floats; dcBlocker: rows pairs;
// d_final may alias d_state).  The workspace starts with four statistics words per row, then the rows' chunk arrays.  The plan
// is the one-row plan, its chunk grown (to a multiple of 8 samples) only where rows * chunks would pass the lane cap.
int64_t rows_min_chunk(int rows, int64_t num, int64_t cap);
AgcPlan agc_rows_plan(int rows, int64_t num, float mu, int run_in);
size_t agc_rows_workspace_bytes(int rows, int64_t num);
void launch_agc_rows(hipStream_t s, int rows, int64_t num, float mu, float reference, const float* d_in, int64_t in_stride,
                     float* d_out, int64_t out_stride, const float* d_state, float* d_final, void* d_ws, int run_in);
DcPlan dc_rows_plan(int rows, int64_t num, int run_in);
size_t dc_blocker_rows_workspace_bytes(int rows, int64_t num);
void launch_dc_blocker_rows(hipStream_t s, int rows, int64_t num, const float* d_in, int64_t in_stride, float* d_out,
                            int64_t out_stride, const float* d_state, float* d_final, void* d_ws, int run_in);
// d_in_iq: row 0's first sample of the range; d_last_iq (may be null: (0, 0)) the rows' predecessors when !has_prev;
// d_last_out (may be null, may alias d_last_iq) receives each row's newest sample
void launch_fm_demod_rows(hipStream_t s, int rows, const float* d_in_iq, int64_t in_stride, float* d_out, int64_t out_stride,
                          int64_t count, bool has_prev, const float* d_last_iq, float* d_last_out);
void rows_launches_add(int launches);
long long rows_launch_count();    // diagnostics: kernel launches of the row forms so far

// Lane-split tiled kernels (kernels_split.hip): every SIMD order of the filter / decimator / resampler families,
// any factor and tap count that fits a tile.  Plain taps (sym: the half taps).  false = not applicable.
bool launch_fir_split(hipStream_t s, const Geom& g, bool cplx, int lanes, ComplexOrder corder, bool sym, const float* d_taps,
                      int ntaps, const float* d_cross_taps, const float* d_in, float* d_out, float gain, bool apply_gain);
bool launch_resample_split(hipStream_t s, const Geom& g, bool cplx, int lanes, ComplexOrder corder, const ResampTable& t,
                           const float* d_groups, const float* d_plain_taps, const float* d_in, float* d_out);

long long split_launch_count();   // diagnostics: launches the lane-split kernels have taken so far

// kernels_fir_rows.hip: the lane-split tile with a row axis (sdrhip_*_run_rows, route 1).  Row r is d_in + r * in_stride ->
// d_out + r * out_stride (floats; even on a complex side); g, taps and tables are the one-row launch's and the same for every row.
// Shapes: those of launch_fir_split / launch_resample_split without their minimum length (g.seamBI >= 0, a SIMD order, 1 .. 64
// chunks, up to 64 groups).  One tile launch, and one fix-up launch when seam_span(g).nseams > 0; false = not this shape, nothing
// launched.  No gain, no u8 input.
struct FirRowsPlan { int cycles_per_tile, tiles_per_row, U, outputs_per_cycle; };
// host arithmetic only (CPU-testable): the plan launch_*_rows follows, and (if asked) the tile plan_tile gives k_split for one such row
bool fir_rows_plan(const Geom& g, int rows, bool cplx, int lanes, ComplexOrder corder, bool sym, int ntaps, FirRowsPlan* rows_plan,
                   FirRowsPlan* one_row_split_plan = nullptr);
bool resample_rows_plan(const Geom& g, int rows, bool cplx, int lanes, ComplexOrder corder, const ResampTable& t, FirRowsPlan* rows_plan,
                        FirRowsPlan* one_row_split_plan = nullptr);
bool launch_fir_rows(hipStream_t s, const Geom& g, int rows, int64_t in_stride, int64_t out_stride, bool cplx, int lanes,
                     ComplexOrder corder, bool sym, const float* d_taps, int ntaps, const float* d_cross_taps, const float* d_in, float* d_out);
bool launch_resample_rows(hipStream_t s, const Geom& g, int rows, int64_t in_stride, int64_t out_stride, bool cplx, int lanes,
                          ComplexOrder corder, const ResampTable& t, const float* d_groups, const float* d_plain_taps, const float* d_in,
                          float* d_out);
long long fir_rows_launch_count();   // diagnostics: banked tile launches
long long fir_rows_fixup_count();    // diagnostics: banked fix-up launches

// kernels_decimate_real.hip: real decimators by 2 / 4 / 8 / 16, AVX / SSE lane order, up to 2048 taps (sym: d_taps = nk half-taps,
// a multiple of 8, g.Lp = 2 nk): 16 / D
// outputs per thread, scalar-loaded taps, rolled walk.  False = not this kernel's shape.
// ncross: taps of the sequential (Cross) outputs when they are not the g.Lp padded ones (a resampler with interpolation 1)
bool launch_decimate_real16_fast(hipStream_t s, const Geom& g, int lanes, const float* d_taps, int nk, const float* d_cross_taps, const float* d_in,
                                 float* d_out, float gain, bool apply_gain, int ncross = 0, bool sym = false);
long long decimate_real16_launch_count();
// kernels_resample_cycle.hip: real resamplers I/D with an odd decimation (I <= 6, D in {3,5,7}), any filter length up to
// 1024 taps per group, AVX / SSE lane order: one thread per polyphase cycle, rolled walk with taps from LDS.  False = not
// this kernel's shape (the caller falls through to the split / generic kernels).
// cplx: complex data in the "RC2" orders (corder CO_X4 / CO_X2: eight / four complex partials)
bool launch_resample_cycle_fast(hipStream_t s, const Geom& g, int lanes, const ResampTable& t, const int* increments, const float* d_groups,
                                const float* d_plain_taps, const float* d_in, float* d_out, bool cplx = false, ComplexOrder corder = CO_SEQ);
long long resample_cycle_launch_count();

// Fast paths (kernels_fast.hip).  Return false when the configuration is not one
// they are specialised for; the caller then uses the generic kernel.
// kernels_chain.hip: fast paths of the low-rate stages
void launch_fm_demod_fast(hipStream_t s, const float* d_in_iq, float* d_out, int64_t count, bool has_prev,
                          float last_re, float last_im);
// real filters (D == 1), AVX order, nk taps walked (half-taps when sym), nk % 8 == 0
// lanes: 8 = AVX order, 4 = SSE order (the same kernel with four lane partials per output)
bool launch_fir_real8_fast(hipStream_t s, const Geom& g, bool sym, const float* d_taps, int nk, const float* d_cross_taps,
                          const float* d_in, float* d_out, float gain, bool apply_gain, int lanes = 8);
// complex filter (D == 1), AVX "RC" order, duplicated taps (2P floats), P % 4 == 0
bool launch_filter_cplx4_fast(hipStream_t s, const Geom& g, const float* d_dup_taps, int P, const float* d_cross_taps,
                              const float* d_in, float* d_out);
// kernels_fast_filter.hip: complex filters of exactly 128 / 64 taps (AVX "RC" order, plain taps) on the tiled decimator with D = 1
bool launch_filter_c4_tile(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const float* d_in,
                           float* d_out);
// kernels_cplx.hip: the same shape on complex data ("RC2" orders of resampleAVXRC / resampleSSERC)
bool launch_resample3c_fast(hipStream_t s, const Geom& g, ComplexOrder order, const ResampTable& t, const int* increments, const float* d_groups,
                            const float* d_plain_taps, const float* d_in, float* d_out);
// d_iq != nullptr: fmDemod fused into the loader (d_iq = decimator output at input 0 of the launch, y_count inputs; d_in is
// then the y buffer, filled only where the lead / tail / seam kernels read it); false = not this shape, nothing launched.
// lanes = 8: AVX order; 4: SSE order (64-float groups, no fused demodulator)
bool launch_resample_3_10_fast(hipStream_t s, const Geom& g, const ResampTable& t, const int* increments,
                               const float* d_groups, const float* d_plain_taps, const float* d_in, float* d_out,
                               const float* d_iq = nullptr, bool iq_has_prev = false, int64_t y_count = 0, int lanes = 8);
// ---- the two fused kernels of the FM chain.  chain.cpp ASKS whether one applies (the predicates below) before it launches or
// times anything; the launchers launch unconditionally.
// The low-rate tail's device tables as both kernels take them (chain.cpp fills them in one place)
struct FmTailTables {
    const float* d_groups; int row_stride;          // resampler: 3 group rows (group g = outputs m = 3c + g), the floats between them
    const float* d_rplain; int ntaps, rLp;          // its plain taps, their unpadded count, numCoeffsR
    const float* d_fhalf; const float* d_fplain;    // audio filter: 64 half-taps, 128 plain taps
    float gain;
    int64_t seam;                                   // block size of every Pipe (0 = contiguous stream)
};
// kernels_tail.hip: the tail both kernels are written for -- 3/10 resampler, 64-float groups, increments {4,3,3}, 64 half-taps.
// Depends on the taps alone: evaluated once, when the chain is created.
bool fm_tail_shape_ok(int ngroups, int nloop, int I, int D, const int* increments, int rLp, int ntaps, int nhalf);
// kernels_tail.hip: fmDemod -> 3/10 resampler -> symmetric filter (* gain) as one kernel (y and z never leave LDS).
// fits (given fm_tail_shape_ok): a buffer of the reference's Pipes is longer than a tile
constexpr int kTailTileOutputs = 2046;   // audio outputs one workgroup of the fused tail kernel produces
bool fm_tail_fused_fits(int rLp, int64_t seam);
void launch_fm_tail_fused(hipStream_t s, const float* d_d, int64_t kd0, int64_t kd1, int64_t ky0, int64_t ky1, float* d_audio,
                          int64_t q0, int64_t q1, const FmTailTables& t);
long long fm_tail_launch_count();   // diagnostics: launches of k_fm_tail
// kernels_tail_rows.hip: the same tile over ROWS of real y (the audio tail behind the AM / narrow-band FM bank, audio_tail.cpp):
// 3/10 resampler -> symmetric filter (* gain), one launch for all rows, the row on the grid's second axis.  Row r's y[0] is its
// stream element y_base, n_y elements readable (others are read as zeros); its outputs [q0, q1) go to d_audio + r * audio_stride.
// Shape and fit are k_fm_tail's: fm_tail_shape_ok and fm_tail_fused_fits.  Launches unconditionally and counts.
void launch_audio_tail_rows(hipStream_t s, const float* d_y, int64_t y_stride, int64_t y_base, int64_t n_y, float* d_audio,
                            int64_t audio_stride, int rows, int64_t q0, int64_t q1, const FmTailTables& t);
long long audio_tail_launch_count();   // diagnostics: launches of k_audio_tail_rows
// kernels_tail_any.hip: the same contract for any down-sampling ratio of a narrow receiver -- I / D, the group length, the tap counts
// and the block are run-time numbers, and a tile may hold any number of buffer boundaries of both stages.  A tile is
// kTailAnyTileOutputs = 840 audio outputs of one row (a multiple of every I <= 8: it starts on a polyphase cycle).
// audio_tail_any_fits is the ONE predicate, shape and block: real data, both stages in the AVX order (8 lanes), a symmetric filter of
// factor 1 and at most 128 prepared taps; I <= 8 groups (gcd(I, D) = 1) of at most 64 padded floats, Lp >= D; a tile's y window --
// D * (ceil((840 + Lf - 1) / I) - 1) + pre[I - 1] + nloop + 8 floats -- within kTailAnyWindowFloats (D / I up to about 5); block 0 or
// any block sdrhip_audio_tail_create admits (block * I >= Lp, block >= Lf: there is no tighter lower bound) up to 2^27.
// launch_audio_tail_rows_any launches unconditionally and counts; t.d_fhalf / t.d_fplain hold s.fLp / 2 and s.fLp taps.
constexpr int kTailAnyTileOutputs = 840, kTailAnyMaxFilter = 128, kTailAnyMaxGroup = 64, kTailAnyMaxInterp = 8, kTailAnyWindowFloats = 5120;
struct TailAnyShape {
    bool cplx; int rlanes, flanes; bool fsym; int ffactor;      // data and orders of the two descriptors
    int I, D, ngroups, nloop, row_stride, ntaps, rLp;           // the resampler
    const int* increments;                                      // per group, from group 0 (ngroups of them)
    int fLp;                                                    // the filter's prepared length (2 x half-taps)
};
bool audio_tail_any_fits(const TailAnyShape& s, int64_t block);
void launch_audio_tail_rows_any(hipStream_t st, const float* d_y, int64_t y_stride, int64_t y_base, int64_t n_y, float* d_audio,
                                int64_t audio_stride, int rows, int64_t q0, int64_t q1, const TailAnyShape& s, const FmTailTables& t);
long long audio_tail_any_launch_count();   // diagnostics: launches of k_audio_tail_rows_any
// kernels_small.hip: the WHOLE chain (u8 IQ -> /8 decimator -> fmDemod -> 3/10 resampler -> symmetric filter * gain) as one
// kernel for launch-bound runs; d_in holds samples [s0, s0 + n_in).  tile_outputs: audio outputs per workgroup (0 = chosen
// from the size of the run, < 0 = the largest).  fits (given fm_tail_shape_ok): /8 decimator with 128 padded taps in the AVX
// order and exactly pre-scaled taps, seam block of at least 192, 16-byte aligned d_in, s0 a multiple of 8
bool fm_chain_small_fits(int dD, int dP, ComplexOrder order, bool scaled_taps, int64_t seam, const void* d_in, int64_t s0);
// d_osc != nullptr: the tuned kernel -- the oscillator (`period` (re, im) pairs, indexed by the absolute stream index) is mixed into
// the converted samples in the tile loader, as kernels_tuner.hip does; d_dtaps is then the PLAIN prepared taps (the mix rounds on the
// fully converted sample, so the 1/128 cannot move into the taps: pass scaled_taps = true to the predicate), and last_tap_zero may
// only be set when no mixed sample can overflow
void launch_fm_chain_small(hipStream_t s, const uint8_t* d_in, int64_t s0, int64_t n_in, float* d_audio, int64_t q0, int64_t q1,
                           const float* d_dtaps, bool last_tap_zero, const FmTailTables& t, int tile_outputs,
                           const float* d_osc = nullptr, int period = 0);
long long fm_chain_small_launch_count();   // diagnostics: launches of the one-kernel chain so far (tuned ones included)
long long fm_chain_small_tuned_launch_count();   // ... and those of the tuned kernel alone
// The receiver bank (sdrhip_fm_bank_run): `stations` tuned chains over ONE input in one launch of that kernel with a station axis in
// the grid.  d_tables holds every station's oscillator table, station j's `periods[j]` (re, im) pairs from pair offsets[j] on; its
// audio outputs [q0, q1) go to d_audio + j * audio_stride.  d_dtaps: the PLAIN prepared taps; last_tap_zero only when no mixed sample
// of ANY station can overflow.  tile_outputs: 0 = chosen from stations * outputs.  fits: fm_chain_small_fits (scaled_taps = true) and
// fm_chain_small_bank_fits, which says whether the grid exists (at most 65535 tiles).  Launches of it count on their own.
constexpr int kFmBankMaxStations = 32;
bool fm_chain_small_bank_fits(int64_t q0, int64_t q1, int stations, int tile_outputs);
void launch_fm_chain_small_bank(hipStream_t s, const uint8_t* d_in, int64_t s0, int64_t n_in, float* d_audio, int64_t audio_stride,
                                int64_t q0, int64_t q1, const float* d_dtaps, bool last_tap_zero, const FmTailTables& t, int tile_outputs,
                                const float* d_tables, int stations, const int* offsets, const int* periods);
long long fm_chain_small_bank_launch_count();
// abi_device.cpp: the short-seamed-launch scale v (sdrhip_set_small_launch_outputs)
int small_launch_outputs();

// last_tap_zero: tap P-1 is the zero the constructor padded the filter with (lets the u8 path skip its MACs)
bool launch_decimate_c4_fast(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps,
                             const void* d_in, bool in_is_u8, float* d_out, bool last_tap_zero = false);
// kernels_systolic.hip (round 4): the One outputs of a decimate-by-8, 128-tap, AVX-order launch by the register-resident systolic
// walk (d_taps: plain taps, pre-scaled by 1/128 for u8 input).  false = not this shape / too small, nothing launched.
// seams_done (with d_cross_taps, the plain taps of the sequential outputs): set when the launch also computed its Cross outputs
// (fix-up workgroups interleaved into the same launch, round 6) -- the caller then skips its fix-up launch.
bool launch_decimate_c4_systolic(hipStream_t s, const Geom& g, const float* d_taps, int P, const void* d_in, bool in_is_u8, float* d_out,
                                 bool last_tap_zero, const float* d_cross_taps = nullptr, bool* seams_done = nullptr);
void systolic_plan(int count, int* nstrips, int* nwhole);   // host arithmetic of the strip cut (CPU-testable)
void set_systolic(int mode);        // 0 = the tile kernel everywhere, 1 = the systolic kernel wherever its shape fits, 2 (default) = by launch size
long long systolic_launch_count();  // diagnostics
long long systolic_plain_launch_count();  // diagnostics: launches with plain (not non-temporal) cfloat loads
long long decimator_crossfix_launch_count();  // diagnostics: seam fix-ups of launch_decimate_c4_fast run as a launch of their own
long long generic_u8_launch_count();  // abi_device.cpp, diagnostics: u8 launches of a complex stage that no u8-fused tiled kernel took
long long fused_demod_launch_count();  // abi_device.cpp, diagnostics: resampler launches with fmDemod in their tile loader
// kernels_fast_orders.hip: the same tiled decimator for the SSE "RC" and the "RC2" summation orders (CO_L2, CO_X4, CO_X2)
bool launch_decimate_c_orders_fast(hipStream_t s, const Geom& g, ComplexOrder order, const float* d_plain_taps, int P,
                                   const float* d_cross_taps, const void* d_in, bool in_is_u8, float* d_out);

// The input of the tuner family: cfloat, interleaved u8 IQ (RTL-SDR: (u - 128) / 128) or interleaved int16 IQ (BladeRF: s / 2048).
// Host code passes it as an argument, kernels take it as an `int FMT` template argument.
enum InFmt : int { IN_CF32 = 0, IN_U8 = 1, IN_I16 = 2 };
constexpr int in_fmt_bytes(int f) { return f == IN_U8 ? 2 : f == IN_I16 ? 4 : 8; }      // per complex sample

// kernels_tuner.hip: the tuner = multiplication by a periodic complex oscillator (d_osc: `period` (re, im) pairs, indexed by the
// ABSOLUTE stream index mod period) in front of the complex decimator.  Fused route: the tiled decimator with the mix in its loader,
// AVX "RC" order, decimation 4 / 8 / 16, up to 128 prepared taps (d_plain_taps, never pre-scaled), 16-byte aligned tile starts;
// Cross outputs in the tile kernel for short launches, else by a fix-up launch over seam_span(g).  false = not this shape, nothing launched.
// int16 input has no one-row kernel: it is launch_tuner_bank with one channel (table offset 0, counts_as_bank = false).
bool launch_tuner_fused(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                        InFmt fmt, float* d_out, const float* d_osc, int period);
// the conditions launch_tuner_fused checks, for callers that plan before they launch (chain.cpp); only the alignment of d_out counts.
// The first window lies at d_in + in_fmt_bytes(fmt) * x0 and is 16-byte aligned; int16 also wants x0 >= 0 and d_in 4-byte aligned.
bool tuner_fused_fits(const Geom& g, int P, bool has_cross_taps, const void* d_in, InFmt fmt, const void* d_out, int period);
// two-pass route, first pass: d_out[i] = mixed sample i of d_in, i < n < 2^31; ph0 = phase of sample 0
void launch_tuner_mix(hipStream_t s, const void* d_in, InFmt fmt, float* d_out, int64_t n, const float* d_osc, int period, int ph0);
long long tuner_fused_launch_count();   // diagnostics: launches of the one-row tile kernel (k_tuner_c4: cfloat and u8)
// kernels_tuner_bank.hip: the tuner bank (sdrhip_tuner_bank_run) -- `channels` tuners of ONE decimator over ONE input in one launch of
// the fused tile kernel with a channel axis (flat grid, the channel fastest).  d_tables holds every channel's oscillator table,
// channel j's `periods[j]` (re, im) pairs from pair offsets[j] on; its outputs go to d_out + j * out_stride floats (out_stride even,
// and at least 2 g.count when there is more than one channel).  Shapes, taps and Cross outputs as launch_tuner_fused, fit predicate
// tuner_fused_fits; false = not this shape, nothing launched.  A launch counts once, its fix-up launch not at all; counts_as_bank =
// false is the one-row int16 tuner's launch, which counts as an int16 launch only.
constexpr int kTunerBankMaxChannels = 32;
bool launch_tuner_bank(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                       InFmt fmt, float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets,
                       const int* periods, bool counts_as_bank);
// What a kernel of the bank stores per finished output (`int OUT` template argument beside FMT): the complex value, or its
// Data.Complex magnitude as one float (am.hpp: am_magnitude) -- the AM bank's envelope form.
// OUT_FM: fm_phase (demod.hpp) of the finished output and its predecessor as one float -- the narrow-band FM bank's form.
enum OutKind : int { OUT_IQ = 0, OUT_ENV = 1, OUT_FM = 2 };
// launch_tuner_bank's launch set in the envelope form (am_bank.cpp): row j is g.count FLOATS at d_out + j * out_stride, any
// out_stride >= g.count (odd ones included) when there is more than one channel, d_out at any float address.  Shapes and input
// alignment as launch_tuner_bank; false = not this shape, nothing launched.  Counts in am_bank_launch_count (int16 input also in
// tuner_i16_launch_count) and in no other counter; its fix-up launch counts in am_bank_fixup_launch_count.
bool launch_am_bank(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                    InFmt fmt, float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets,
                    const int* periods);
// launch_tuner_bank_cross in the envelope form: the Cross part of a ragged push of the AM bank's Pipe (pipes.cpp).  Float rows, any
// out_stride >= g.count with more than one channel, d_out at any float address; false = refused, nothing launched.
bool launch_am_bank_cross(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, InFmt fmt, float* d_out,
                          int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods);
long long am_bank_cross_launch_count();   // diagnostics: launches of the all-Cross envelope kernel
// launch_tuner_bank's tile launch in the fmDemod form (nfm_bank.cpp): row j is g.count FLOATS at d_out + j * out_stride, output k =
// fm_phase(y[k], y[k - 1]); d_state = `channels` (re, im) pairs, channel j's decimated output k_begin - 1 (null = zeros), d_final
// (null = not wanted) receives output k_begin + count - 1.  The two must not overlap (the caller checks).  ONE launch: every Cross
// output is computed in the tile, for any seam in [Lp, 2^30); a longer seam is refused.  Shapes and input alignment as
// launch_tuner_bank; false = not this shape, nothing launched.  Counts in nfm_bank_launch_count (int16 input also in
// tuner_i16_launch_count) and in no other counter.
bool launch_nfm_bank(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                     InFmt fmt, float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets,
                     const int* periods, const float* d_state, float* d_final);
// launch_tuner_bank_cross in the fmDemod form: every output Cross, thread t computes y[t] and y[t - 1] (the Pipe's ragged boundary)
bool launch_nfm_bank_cross(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, InFmt fmt, float* d_out,
                           int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods,
                           const float* d_state, float* d_final);
long long nfm_bank_launch_count();        // diagnostics: fmDemod-form tile launches, every format
long long nfm_bank_cross_launch_count();  // diagnostics: launches of the all-Cross fmDemod-form kernel
long long am_bank_launch_count();         // diagnostics: envelope tile launches, every format
long long am_bank_fixup_launch_count();   // diagnostics: envelope fix-up launches
long long tuner_bank_launch_count();    // diagnostics: banked launches, every format
long long tuner_i16_launch_count();     // diagnostics: int16 launches of the tile kernel, bank or one-row
// kernels_narrow.hip: the narrow-channel bank's kernel (narrow_bank.cpp) -- the complex SECOND decimator over the `channels` rows the
// tuner bank has written, with the demodulator as its store.  g is the second decimator's launch (g.in_base = the stage-1 index of
// every row's d_in[0]); row j is d_in + j * in_stride floats, 16-byte aligned (in_stride a multiple of 4), n_in complex samples
// readable; its outputs go to d_out + j * out_stride as one float each: am_magnitude (NARROW_ENV) or fm_phase against the output
// before (NARROW_FM: d_state / d_final as launch_nfm_bank's, not overlapping).  Every Cross output is computed in the tile.  Serves
// the AVX "RC" order, factor <= 16, up to 128 prepared taps (a multiple of 4), seam 0 or in [Lp, 2^30); ONE launch, counted;
// false = not this shape or a window outside the rows, nothing launched.
enum NarrowForm : int { NARROW_ENV = 0, NARROW_FM = 1 };
constexpr int kNarrowTileThreads = 256, kNarrowMaxFactor = 16, kNarrowMaxTaps = 128;
// outputs a tile advances by: NARROW_FM's tiles overlap by one output (the predecessor of a tile's first phase)
__host__ __device__ constexpr int narrow_tile_advance(int form) { return form == NARROW_FM ? kNarrowTileThreads - 1 : kNarrowTileThreads; }
int narrow_tile_count(int form, int count);
bool narrow_rows_fits(const Geom& g, ComplexOrder corder, int channels, const float* d_in, int64_t in_stride);
bool launch_narrow_rows(hipStream_t s, const Geom& g, int form, ComplexOrder corder, const float* d_plain_taps, const float* d_in,
                        int64_t in_stride, int64_t n_in, float* d_out, int64_t out_stride, int channels, const float* d_state, float* d_final);
long long narrow_bank_launch_count();     // diagnostics: launches of k_narrow_rows
// Outputs [g.k_begin, g.k_begin + g.count) of every channel in the reference's sequential order, all of them (g.seamBI is not read):
// the Cross part of a ragged push of the tuner bank's Pipe (pipes.cpp), one thread per (channel, output).  The refusals of
// launch_tuner_bank for channels and stride, no alignment beyond the element's own; false = refused, nothing launched.
bool launch_tuner_bank_cross(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, InFmt fmt, float* d_out,
                             int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods);
long long tuner_bank_cross_launch_count();   // diagnostics: launches of the all-Cross kernel, every format
// kernels_small.hip: launch_fm_chain_small_bank on 16-bit signed IQ (sdrhip_fm_bank_run_i16): the tuned one-kernel chain with a station
// axis and an int16 phase 0 (small_i16.hpp).  fm_chain_small_i16_fits: the tuned chain's shape and seam conditions with int16's
// alignment (d_in 16-byte aligned, s0 a multiple of 4); the grid's condition is fm_chain_small_bank_fits.  A launch counts in
// fm_chain_small_bank_launch_count AND in the int16 counter.
bool fm_chain_small_i16_fits(int dD, int dP, ComplexOrder order, int64_t seam, const void* d_in, int64_t s0);
void launch_fm_chain_small_bank_i16(hipStream_t s, const int16_t* d_in, int64_t s0, int64_t n_in, float* d_audio, int64_t audio_stride,
                                    int64_t q0, int64_t q1, const float* d_dtaps, bool last_tap_zero, const FmTailTables& t, int tile_outputs,
                                    const float* d_tables, int stations, const int* offsets, const int* periods);
long long fm_chain_small_bank_i16_launch_count();

}  // namespace sdrhip
