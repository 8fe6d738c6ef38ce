// audio_tail.cpp -- the audio stages behind the AM and narrow-band FM banks over rows (include/sdr_hip.h, "audio tail"):
//     y rows  >->  firResampler(block)  >->  firFilter(block)  >->  (* gain)
// Route 2 is the definition: sdrhip_resampler_run_rows, sdrhip_filter_run_rows and sdrhip_scale_run through the C ABI, as a caller
// without this object composes them, the z and filter rows in the caller's workspace.  Route 1 is k_audio_tail_rows
// (kernels_tail_rows.hip): one launch, no workspace, the shape and fit of the FM chain's fused tail.  Route 0 = auto: the measured
// rule below; where that rule does not take it, k_audio_tail_rows_any (kernels_tail_any.hip: any down-sampling ratio, any number of
// seams per tile) by sdrhip_audio_tail_set_general's mode and its own measured rule.  The plan functions are host arithmetic
// (tail_plan.hpp, shared with chain.cpp) and need no device.  Every refusal comes before any device work, the descriptors' first-use
// upload included.
#include <atomic>

#include "descriptors.hpp"
#include "tail_plan.hpp"

using namespace sdrhip;

struct sdrhip_audio_tail {
    sdrhip_resampler* res = nullptr;     // real, owned
    sdrhip_filter* fil = nullptr;        // symmetric real, owned
    float gain = 1.0f;
    int64_t block = 0;                   // the one block size of every Pipe of the tail (0 = contiguous)
    bool fm_tail = false;                // the shape k_audio_tail_rows is written for (fm_tail_shape_ok, AVX orders)
    std::atomic<int> route{0};
    TailAnyShape any = {};               // what audio_tail_any_fits reads (increments: the resampler's, owned above)
    std::atomic<int> general{0};         // route 0 only: 0 = the measured rule, 1 = k_audio_tail_rows_any wherever it fits, 2 = never
    ~sdrhip_audio_tail()
    {
        sdrhip_resampler_destroy(res);
        sdrhip_filter_destroy(fil);
    }
    int64_t first_y(int64_t q) const { return tail_first_y(*res, q); }
    int64_t end_y(int64_t q) const { return tail_end_y(*res, *fil, q); }
    bool fused_fits() const { return fm_tail && fm_tail_fused_fits(res->Lp, block); }
    bool general_fits() const { return audio_tail_any_fits(any, block); }
    // floats of a z row / a filter row that any range inside n_y readable inputs can need: a resampler output per D / I inputs
    int64_t max_outputs(int64_t n_y) const { return n_y * res->I / res->D + 2; }
};

namespace {

enum { ROUTE_AUTO = 0, ROUTE_FUSED = 1, ROUTE_COMPOSED = 2 };
enum { GENERAL_AUTO = 0, GENERAL_ALWAYS = 1, GENERAL_NEVER = 2 };

// The auto rule (sdr_hip.h states it beside the routes; tools/audio_tail_bench.py, profiles/audio_tail_bench.txt).  Measured:
// 1 / 2 / 8 / 32 rows x 153 / 2458 / 39322 / 314574 audio outputs per row, block 0 and 8192, in three row layouts, route 1 against
// route 2 alternating in one process, 7 rounds.  The layouts: both sides back to back (y_stride == n_y, audio_stride == q1 - q0, or
// one row); the y rows strided and the audio rows back to back (the audio Pipes' layout: a padded rows buffer behind a carried
// history); the audio rows strided.  kFused[layout][seamed][rows][size]: route 1's slowest round was below route 2's fastest at
// that point.  A run between measured row counts or sizes is fused only where every measured neighbour is; a block > 0 other than
// 8192 takes both block tables; fewer than 153 or more than 314574 outputs per row and more than 32 rows were not measured and are
// composed.
enum { LAYOUT_CONTIGUOUS = 0, LAYOUT_Y_STRIDED = 1, LAYOUT_AUDIO_STRIDED = 2 };
constexpr int64_t kAutoSizes[4] = {153, 2458, 39322, 314574};
constexpr int kAutoRows[4] = {1, 2, 8, 32};
#define ALL_AHEAD {{true, true, true, true}, {true, true, true, true}, {true, true, true, true}, {true, true, true, true}}
constexpr bool kFused[3][2][4][4] = {       // route 1 was ahead at every point of the sweep
    /* back to back:   block 0, 8192 */ {ALL_AHEAD, ALL_AHEAD},
    /* y strided:      block 0, 8192 */ {ALL_AHEAD, ALL_AHEAD},
    /* audio strided:  block 0, 8192 */ {ALL_AHEAD, ALL_AHEAD},
};
#undef ALL_AHEAD

int layout_of(int rows, int64_t y_stride, int64_t n_y, int64_t audio_stride, int64_t nq)
{
    if (rows == 1) return LAYOUT_CONTIGUOUS;          // one row has no stride
    return audio_stride != nq ? LAYOUT_AUDIO_STRIDED : y_stride != n_y ? LAYOUT_Y_STRIDED : LAYOUT_CONTIGUOUS;
}

bool auto_fuses(int rows, int64_t outputs, int64_t block, int layout)
{
    if (rows < kAutoRows[0] || rows > kAutoRows[3] || outputs < kAutoSizes[0] || outputs > kAutoSizes[3]) return false;
    int rhi = 0, shi = 0;
    while (kAutoRows[rhi] < rows) rhi++;
    while (kAutoSizes[shi] < outputs) shi++;
    const int rlo = kAutoRows[rhi] == rows ? rhi : rhi - 1, slo = kAutoSizes[shi] == outputs ? shi : shi - 1;
    for (int seamed = 0; seamed < 2; seamed++) {
        if (block == 0 ? seamed == 1 : (block == 8192 && seamed == 0)) continue;
        for (int r = rlo; r <= rhi; r++)
            for (int i = slo; i <= shi; i++)
                if (!kFused[layout][seamed][r][i]) return false;
    }
    return true;
}

// The general kernel's rule (mode 0; tools/audio_tail_any_bench.py, profiles/audio_tail_any_bench.txt).  The sweep: 1 / 2 / 8 / 32 rows x
// 51 / 204 / 3276 / 52428 audio outputs per row, block 0 and 256, the three layouts above, on two tails -- 4/5 x 63 taps and 2/5 x 127
// taps, each with 2 x 64 audio taps -- k_audio_tail_rows_any against route 2 alternating in one process, 7 rounds.
// kGeneral[shape][layout][seamed][rows][size]: the general kernel's slowest round was below route 2's fastest at that point.  Between
// measured row counts or sizes every measured neighbour must be ahead; a block > 0 other than 256 takes both block tables; any other
// tail shape, fewer than 51 or more than 52428 outputs per row and more than 32 rows were not measured and are composed.  A tail of
// k_audio_tail_rows' shape never takes the general kernel under this rule: its own rule above has measured it.
// Measured: the general kernel was ahead at all 192 points -- general / composed, medians: 4/5 x 63 back to back and y strided 0.37 ..
// 0.78 (one row of 51 outputs, block 256: 7.6 against 11.3 us; 32 rows of 52428: 52 against 87 us), audio strided 0.05 .. 0.77;
// 2/5 x 127 back to back and y strided 0.56 .. 0.96 (the closest point: 32 rows of 51 outputs, block 0, 8.9 against 9.3 us, every
// round of either within 0.1 us of its median), audio strided 0.06 .. 0.87.
constexpr int64_t kGeneralSizes[4] = {51, 204, 3276, 52428};
#define ALL_AHEAD {{true, true, true, true}, {true, true, true, true}, {true, true, true, true}, {true, true, true, true}}
constexpr bool kGeneral[2][3][2][4][4] = {       // the general kernel was ahead at every point of the sweep
    /* 4/5 x 63:  back to back, y strided, audio strided; block 0, 256 */ {{ALL_AHEAD, ALL_AHEAD}, {ALL_AHEAD, ALL_AHEAD}, {ALL_AHEAD, ALL_AHEAD}},
    /* 2/5 x 127: back to back, y strided, audio strided; block 0, 256 */ {{ALL_AHEAD, ALL_AHEAD}, {ALL_AHEAD, ALL_AHEAD}, {ALL_AHEAD, ALL_AHEAD}},
};
#undef ALL_AHEAD

// the swept tails: their ratio, taps and 2 x 64 audio taps (-1: another shape)
int general_shape_of(const TailAnyShape& s)
{
    if (s.fLp != 128 || s.D != 5) return -1;
    return s.I == 4 && s.ntaps == 63 ? 0 : s.I == 2 && s.ntaps == 127 ? 1 : -1;
}

bool auto_general(int shape, int rows, int64_t outputs, int64_t block, int layout)
{
    if (shape < 0 || rows < kAutoRows[0] || rows > kAutoRows[3] || outputs < kGeneralSizes[0] || outputs > kGeneralSizes[3]) return false;
    int rhi = 0, shi = 0;
    while (kAutoRows[rhi] < rows) rhi++;
    while (kGeneralSizes[shi] < outputs) shi++;
    const int rlo = kAutoRows[rhi] == rows ? rhi : rhi - 1, slo = kGeneralSizes[shi] == outputs ? shi : shi - 1;
    for (int seamed = 0; seamed < 2; seamed++) {
        if (block == 0 ? seamed == 1 : (block == 256 && seamed == 0)) continue;
        for (int r = rlo; r <= rhi; r++)
            for (int i = slo; i <= shi; i++)
                if (!kGeneral[shape][layout][seamed][r][i]) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int sdrhip_audio_tail_create(sdrhip_audio_tail** t, int order, int interpolation, int decimation, const float* resamp_taps,
                             int n_resamp_taps, const float* audio_half_taps, int n_audio_half, float gain, int64_t block)
{
    SDRHIP_REQUIRE(t != nullptr, "sdrhip_audio_tail_create");
    *t = nullptr;
    SDRHIP_REQUIRE(block >= 0, "sdrhip_audio_tail_create");
    sdrhip_audio_tail* a = new sdrhip_audio_tail();
    int rc = sdrhip_resampler_create(&a->res, order, 0, interpolation, decimation, resamp_taps, n_resamp_taps);
    if (rc == SDRHIP_OK) rc = sdrhip_filter_sym_create(&a->fil, order, audio_half_taps, n_audio_half);
    if (rc == SDRHIP_OK && block != 0 && !(block * a->res->I >= a->res->Lp && a->res->Lp >= a->res->D && block >= a->fil->Lp)) {
        set_error("sdrhip_audio_tail_create: block %lld shorter than a stage's filter (Filter.hs:586,691)", (long long)block);
        rc = SDRHIP_ERR_ARG;
    }
    if (rc != SDRHIP_OK) { delete a; return rc; }
    a->gain = gain;
    a->block = block;
    const ResampDesc& r = *a->res;
    const FirDesc& f = *a->fil;
    a->fm_tail = !r.cplx && r.lanes == 8 && !f.cplx && f.sym && f.lanes == 8 && f.factor == 1 &&
                 fm_tail_shape_ok(r.num_groups, r.nloop, r.I, r.D, r.increments.data(), r.Lp, r.ntaps, f.ntaps_kernel);
    a->any = {r.cplx, r.lanes, f.lanes, f.sym, f.factor, r.I, r.D, r.num_groups, r.nloop, r.row_stride, r.ntaps, r.Lp, r.increments.data(), f.Lp};
    *t = a;
    return SDRHIP_OK;
}

void sdrhip_audio_tail_destroy(sdrhip_audio_tail* t) { delete t; }

int64_t sdrhip_audio_tail_ready(const sdrhip_audio_tail* t, int64_t n_y)
{
    if (!t || n_y < 0) return -1;
    return ready_by_end([t](int64_t q) { return t->end_y(q); }, n_y);
}

int64_t sdrhip_audio_tail_first_input(const sdrhip_audio_tail* t, int64_t q) { return t && q >= 0 ? t->first_y(q) : -1; }

int64_t sdrhip_audio_tail_max_halo(const sdrhip_audio_tail* t)
{
    if (!t) return -1;
    return longest_field([t](int64_t q) { return t->first_y(q); }, [t](int64_t q) { return t->end_y(q); }, t->res->I);
}

int64_t sdrhip_audio_tail_block(const sdrhip_audio_tail* t) { return t ? t->block : -1; }

int sdrhip_audio_tail_shape(const sdrhip_audio_tail* t, int32_t* shape)
{
    SDRHIP_REQUIRE(t != nullptr && shape != nullptr, "sdrhip_audio_tail_shape");
    shape[0] = t->res->I; shape[1] = t->res->D; shape[2] = t->res->Lp; shape[3] = t->fil->Lp;
    return SDRHIP_OK;
}

int sdrhip_audio_tail_fused_fits(const sdrhip_audio_tail* t) { return t ? (t->fused_fits() ? 1 : 0) : SDRHIP_ERR_ARG; }

size_t sdrhip_audio_tail_workspace_bytes(const sdrhip_audio_tail* t, int rows, int64_t n_y)
{
    if (!t || rows < 1 || rows > SDRHIP_ROWS_MAX || n_y < 0) return 0;
    const int64_t n = t->max_outputs(n_y);
    return (size_t)rows * (size_t)(2 * row_floats(n)) * sizeof(float);      // the z rows, then the filter rows
}

int sdrhip_audio_tail_set_route(sdrhip_audio_tail* t, int route)
{
    SDRHIP_REQUIRE(t != nullptr, "sdrhip_audio_tail_set_route");
    SDRHIP_REQUIRE(route >= ROUTE_AUTO && route <= ROUTE_COMPOSED, "sdrhip_audio_tail_set_route");
    t->route.store(route, std::memory_order_relaxed);
    return SDRHIP_OK;
}

long long sdrhip_debug_audio_tail_launches(void) { return audio_tail_launch_count(); }

int sdrhip_audio_tail_general_fits(const sdrhip_audio_tail* t) { return t ? (t->general_fits() ? 1 : 0) : SDRHIP_ERR_ARG; }

int sdrhip_audio_tail_set_general(sdrhip_audio_tail* t, int mode)
{
    SDRHIP_REQUIRE(t != nullptr, "sdrhip_audio_tail_set_general");
    SDRHIP_REQUIRE(mode >= GENERAL_AUTO && mode <= GENERAL_NEVER, "sdrhip_audio_tail_set_general");
    t->general.store(mode, std::memory_order_relaxed);
    return SDRHIP_OK;
}

long long sdrhip_debug_audio_tail_general_launches(void) { return audio_tail_any_launch_count(); }

int sdrhip_audio_tail_run_rows(const sdrhip_audio_tail* t, void* stream, const float* d_y, int64_t y_stride, int64_t y_base, int64_t n_y,
                               float* d_audio, int64_t audio_stride, int rows, int64_t q0, int64_t q1, void* d_workspace,
                               size_t workspace_bytes)
{
    const char* what = "sdrhip_audio_tail_run_rows";
    SDRHIP_REQUIRE(t != nullptr, what);
    SDRHIP_REQUIRE(rows >= 1 && rows <= SDRHIP_ROWS_MAX, what);
    const int route = t->route.load(std::memory_order_relaxed);
    SDRHIP_REQUIRE(route >= ROUTE_AUTO && route <= ROUTE_COMPOSED, what);
    SDRHIP_REQUIRE(q0 >= 0 && q1 >= q0 && y_base >= 0 && n_y >= 0, what);
    if (q1 == q0) return SDRHIP_OK;
    const int64_t nq = q1 - q0, nz = nq + t->fil->Lp - 1;
    SDRHIP_REQUIRE(nz < (int64_t)0x7fffffff, what);
    SDRHIP_REQUIRE(t->first_y(q0) >= y_base && t->end_y(q1 - 1) <= y_base + n_y, what);      // the receptive field is readable
    SDRHIP_REQUIRE(d_y != nullptr && d_audio != nullptr && d_y != d_audio, what);
    SDRHIP_REQUIRE(rows == 1 || (audio_stride >= nq && y_stride >= n_y), what);
    const bool fits = t->fused_fits();
    if (route == ROUTE_FUSED && !fits) {
        set_error("%s: route 1 on a tail the fused kernel does not serve (shape or block)", what);
        return SDRHIP_ERR_ARG;
    }
    const int layout = layout_of(rows, y_stride, n_y, audio_stride, nq);
    const bool fused = fits && (route == ROUTE_FUSED || (route == ROUTE_AUTO && auto_fuses(rows, nq, t->block, layout)));
    // route 0 only, behind the existing rule: the general kernel by its mode (mode 0 never on k_audio_tail_rows' own shape)
    const int mode = t->general.load(std::memory_order_relaxed);
    const bool general = !fused && route == ROUTE_AUTO && mode != GENERAL_NEVER && t->general_fits() &&
                         (mode == GENERAL_ALWAYS || (!t->fm_tail && auto_general(general_shape_of(t->any), rows, nq, t->block, layout)));
    // routes 0 and 2 ask for the workspace whichever way auto goes: what a call needs does not depend on a measured table
    SDRHIP_REQUIRE(route == ROUTE_FUSED || (d_workspace != nullptr && workspace_bytes >= sdrhip_audio_tail_workspace_bytes(t, rows, n_y)), what);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (fused || general) {
        if ((rc = t->res->ensure_device()) != SDRHIP_OK || (rc = t->fil->ensure_device()) != SDRHIP_OK) return rc;
        const FmTailTables tt = {t->res->d_groups, t->res->row_stride, t->res->d_plain, t->res->ntaps, t->res->Lp,
                                 t->fil->d_taps, t->fil->d_cross, t->gain, t->block};
        if (fused) launch_audio_tail_rows(s, d_y, y_stride, y_base, n_y, d_audio, audio_stride, rows, q0, q1, tt);
        else launch_audio_tail_rows_any(s, d_y, y_stride, y_base, n_y, d_audio, audio_stride, rows, q0, q1, t->any, tt);
        SDRHIP_CHECK_HIP(hipGetLastError());
        return SDRHIP_OK;
    }
    // the composition: z outputs [q0, q1 + Lf - 1) of every row, then the filter's [q0, q1), then the gain
    // (the filter rows back to back, so that one sdrhip_scale_run takes them all into audio rows that are back to back too)
    const int64_t zs = row_floats(nz), fs = nq;
    if ((size_t)rows * (size_t)(zs + fs) * sizeof(float) > workspace_bytes) {
        set_error("%s: the workspace bound does not cover this range", what);
        return SDRHIP_ERR_STATE;
    }
    float* d_z = static_cast<float*>(d_workspace);
    float* d_f = d_z + (int64_t)rows * zs;
    // The row forms on their banked route wherever it serves the shape, else row by row -- not on their auto route: the definition
    // is "all rows in the existing launch sets", the same launches whatever the rows and the length, and the row forms' auto rule was
    // read from other shapes (a 31-tap resampler, 2 x 32 audio taps) and sends one row and everything outside its sweep row by row,
    // which would make the yardstick route 1 is measured against depend on a table measured elsewhere.
    const int r_route = resamp_rows_banked(t->res, rows, q0, q0 + nz, t->block) ? 1 : 2;
    const int f_route = fir_rows_banked(t->fil, rows, q0, q1, t->block) ? 1 : 2;
    if ((rc = sdrhip_resampler_run_rows(t->res, stream, d_y, y_stride, y_base, d_z, zs, rows, q0, q0 + nz, t->block, t->block, r_route)) != SDRHIP_OK)
        return rc;
    if ((rc = sdrhip_filter_run_rows(t->fil, stream, d_z, zs, q0, d_f, fs, rows, q0, q1, t->block, f_route)) != SDRHIP_OK) return rc;
    if (rows == 1 || audio_stride == nq) return sdrhip_scale_run(stream, t->gain, d_f, d_audio, (int64_t)rows * nq);
    for (int r = 0; r < rows; r++)
        if ((rc = sdrhip_scale_run(stream, t->gain, d_f + r * fs, d_audio + r * audio_stride, nq)) != SDRHIP_OK) return rc;
    return SDRHIP_OK;
}

}  // extern "C"
