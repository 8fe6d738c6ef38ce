// narrow_bank.cpp -- the narrow-channel bank of include/sdr_hip.h: tuner -> firDecimator D1 -> firDecimator D2 -> demodulator for every
// channel of one capture.
//
// Definition (and route 2, composed): sdrhip_tuner_bank_run* over the stage-1 outputs [k_begin D2, (k_end - 1) D2 + Lp2) into complex
// rows of the workspace, sdrhip_decimator_run_rows (its auto route) into a second set of complex rows, then sdrhip_am_demod_run_rows
// or sdrhip_fm_demod_run_rows, and with dc_block sdrhip_dc_blocker_run_rows from and to d_dc_state with a workspace and the default
// run-in -- the calls a caller makes without this object, through the C ABI, unchanged.
// Route 1 (fused): the same tuner bank call into the same 16-byte aligned rows, then ONE launch of k_narrow_rows (kernels_narrow.hip)
// for all channels: the second decimator with the demodulator as its store, every Cross output computed in the tile; with dc_block
// the envelope rows pass through the workspace into the same sdrhip_dc_blocker_run_rows call (it refuses d_in == d_out).  Nothing is
// argued anew: the stage-1 rows are the tuner bank's on both routes, a One output is summed in the CO_L4 order of the generic kernel,
// a Cross output in the sequential order of the fix-up kernels, the magnitude is am.hpp's and the phase demod.hpp's device function.
#include "descriptors.hpp"

namespace sdrhip {
namespace {

// auto, read from tools/narrow_bank_bench.py (profiles/narrow_bank_bench.txt) by the project's criterion: route 1 where its SLOWEST of 7
// rounds was below route 2's FASTEST, for ALL THREE input types.  The sweep: 1 / 2 / 8 / 32 channels x launches of 8192, 2^17, 2^20 and
// 2^24 input samples (stage 1: 128 taps / 8, so 1009 / 16369 / 131057 / 2097137 stage-1 outputs a channel), u8 / cfloat / int16, the
// envelope form without and with dcBlocker and the fmDemod form, second decimators 24 taps / 4 and 61 taps / 5, (seam_block,
// seam_block2) = (0, 0) and (8192, 1024); 576 points.  kNarrowAuto holds the transcript's closing tables: one mask per channel count,
// bit i = the i-th size is ahead.  Without dcBlocker route 1 is ahead at every point up to 2^20 samples (0.35 .. 0.94 of route 2's
// time: 10.8 against 13.7 us for one channel at 8192 samples of u8, envelope, 24 / 4) and level at 2^24 with 8 and 32 channels at
// factor 4 (0.97 .. 1.04); with dcBlocker its walk is most of either route: 0.81 .. 1.08, level from 2^20 samples on, 49 of 64
// cells ahead.  Windows of 0.05 s (a first sweep with 0.02 s lost cells to single slow rounds and was replaced).
// The rule's size is count, the stage-2 outputs a channel, against the measured launches' 247 / 4087 / 32759 / 524279 (factor 4) and
// 190 / 3262 / 26199 / 419415 (factor 5).  A count at a measured size takes that bit; between two measured sizes both neighbours
// must be ahead; a channel count between two measured ones takes both neighbours.
// Not measured, hence route 2: counts below the smallest or above the largest measured one, factors other than 4 and 5, more prepared taps than the measured
// decimator of that factor (24 and 64; fewer taps are held to the rule unmeasured: the same loads, less arithmetic on both routes),
// seam_block2 other than 0 and 1024.  seam_block and the tuner bank's factor and taps are not told apart: stage 1 is the same call on
// both routes.
constexpr int64_t kNarrowAutoCounts[2][4] = {{247, 4087, 32759, 524279}, {190, 3262, 26199, 419415}};
constexpr int kNarrowAutoChannels[4] = {1, 2, 8, 32};
constexpr int kNarrowAutoFactor[2] = {4, 5}, kNarrowAutoTaps[2] = {24, 64};
constexpr int64_t kNarrowAutoSeam2 = 1024;
// [form: envelope, envelope + dcBlocker, fmDemod][decimator: 24 / 4, 61 / 5][seams: none, (8192, 1024)][channels: 1, 2, 8, 32]
constexpr unsigned char kNarrowAuto[3][2][2][4] = {
    {{{0xf, 0xf, 0x7, 0x7}, {0xf, 0xf, 0x7, 0x7}}, {{0xf, 0xf, 0xf, 0xf}, {0xf, 0xf, 0xf, 0xf}}},
    {{{0x9, 0x7, 0x3, 0x7}, {0xd, 0xf, 0x7, 0x7}}, {{0x9, 0xd, 0xb, 0xb}, {0xd, 0xf, 0xf, 0xf}}},
    {{{0xf, 0xf, 0x7, 0x7}, {0xf, 0xf, 0x7, 0x7}}, {{0xf, 0xf, 0xf, 0xf}, {0xf, 0xf, 0xf, 0xf}}},
};

bool narrow_bank_auto(int channels, int form, bool dc, int factor2, int taps2, int64_t seam_block2, int64_t count)
{
    const int di = factor2 == kNarrowAutoFactor[0] ? 0 : factor2 == kNarrowAutoFactor[1] ? 1 : -1;
    if (di < 0 || taps2 > kNarrowAutoTaps[di]) return false;
    if (seam_block2 != 0 && seam_block2 != kNarrowAutoSeam2) return false;
    const int64_t* sizes = kNarrowAutoCounts[di];
    if (channels < kNarrowAutoChannels[0] || channels > kNarrowAutoChannels[3] || count < sizes[0] || count > sizes[3]) return false;
    const unsigned char* row = kNarrowAuto[form == NARROW_FM ? 2 : dc ? 1 : 0][di][seam_block2 != 0];
    int khi = 0, shi = 0;
    while (kNarrowAutoChannels[khi] < channels) khi++;
    while (sizes[shi] < count) shi++;
    const int klo = kNarrowAutoChannels[khi] == channels ? khi : khi - 1, slo = sizes[shi] == count ? shi : shi - 1;
    for (int k = klo; k <= khi; k++)
        for (int i = slo; i <= shi; i++)
            if (!((row[k] >> i) & 1)) return false;
    return true;
}

// stage-1 outputs a run of `count` stage-2 outputs reads
int64_t stage1_count(const FirDesc* d2, int64_t count) { return (count - 1) * d2->factor + d2->Lp; }

size_t dc_bytes(int K, int64_t count, bool dc)
{
    return dc ? (size_t)K * (size_t)row_floats(count) * sizeof(float) + dc_blocker_rows_workspace_bytes(K, count) : 0;
}
// workspace: [stage-1 complex rows | stage-2 complex rows (composed) | envelope rows (dc_block) | dcBlocker's own]
size_t route1_bytes(const NarrowBankDesc* b, int K, int64_t count)
{
    return (size_t)K * 2 * (size_t)row_floats(stage1_count(b->d2, count)) * sizeof(float) + dc_bytes(K, count, b->dc_block != 0);
}
size_t route2_bytes(const NarrowBankDesc* b, int K, int64_t count)
{
    return route1_bytes(b, K, count) + (size_t)K * 2 * (size_t)row_floats(count) * sizeof(float);
}
bool count_ok(const NarrowBankDesc* b, int64_t count)
{
    return count > 0 && count < (int64_t)0x7fffffff && stage1_count(b->d2, count) < (int64_t)0x7fffffff;
}

}  // namespace

// Everything behind the tuner bank, over complex rows that exist: row j is d_rows + j * stride floats (16-byte aligned rows for the
// fused launch), its element 0 is stage-1 output in_base, n_in elements readable.  fused: ONE launch of k_narrow_rows; else
// sdrhip_decimator_run_rows (route 0) into complex rows of the workspace and the demodulator's rows form.  With dc_block the envelope
// rows pass through the workspace into sdrhip_dc_blocker_run_rows.  d_ws: narrow_stage2_bytes, 16-byte aligned.  narrow_bank_run and
// the bank's Pipe (rows_tail, pipes_fir.cpp) both end here.
size_t narrow_stage2_bytes(const NarrowBankDesc* b, int K, int64_t count, bool fused)
{
    return (fused ? 0 : (size_t)K * 2 * (size_t)row_floats(count) * sizeof(float)) + dc_bytes(K, count, b->dc_block != 0);
}

bool narrow_stage2_fits(const NarrowBankDesc* b, int K, const float* d_rows, int64_t stride, int64_t in_base, int64_t k_begin, int64_t k_end,
                        int64_t seam_block2)
{
    return narrow_rows_fits(bank_geom(b->d2, in_base, k_begin, k_end, seam_block2), b->d2->corder, K, d_rows, stride);
}

int narrow_stage2(const NarrowBankDesc* b, hipStream_t s, bool fused, const float* d_rows, int64_t stride, int64_t in_base, int64_t n_in,
                  float* d_out, int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block2, const float* d_state, float* d_final,
                  float* d_dc_state, float* ws, size_t ws_bytes)
{
    const FirDesc* d2 = b->d2;
    const int K = (int)b->tb->ch.size();
    const bool dc = b->dc_block != 0, fm = b->form == NARROW_FM;
    const int64_t count = k_end - k_begin, np = row_floats(count);
    float* rest = ws;
    float* env;          // where the demodulated rows go: d_out, or with dc_block rows of the workspace
    int rc;
    if (fused) {
        env = dc ? rest : d_out;
        if (!launch_narrow_rows(s, bank_geom(d2, in_base, k_begin, k_end, seam_block2), b->form, d2->corder, d2->d_plain, d_rows, stride, n_in, env,
                                dc ? np : out_stride, K, d_state, d_final)) {
            set_error("sdrhip_narrow_bank_run: the fused launch refused a run its predicate admitted");
            return SDRHIP_ERR_STATE;
        }
        SDRHIP_CHECK_HIP(hipGetLastError());
    } else {
        float* iq2 = rest;
        rest = iq2 + (size_t)K * 2 * (size_t)np;
        env = dc ? rest : d_out;
        rc = sdrhip_decimator_run_rows(static_cast<const sdrhip_decimator*>(d2), s, d_rows, stride, in_base, iq2, 2 * np, K, k_begin, k_end,
                                       seam_block2, 0);
        if (rc != SDRHIP_OK) return rc;
        if (fm) rc = sdrhip_fm_demod_run_rows(s, iq2, 2 * np, k_begin, env, out_stride, K, k_begin, k_end, d_state, d_final);
        else rc = sdrhip_am_demod_run_rows(s, iq2, 2 * np, env, dc ? np : out_stride, K, count);
        if (rc != SDRHIP_OK) return rc;
    }
    if (!dc) return SDRHIP_OK;
    float* dcw = env + (size_t)K * (size_t)np;
    return sdrhip_dc_blocker_run_rows(s, env, np, d_out, out_stride, K, count, d_dc_state, d_dc_state, dcw,
                                      ws_bytes - (size_t)(dcw - ws) * sizeof(float), 0);
}

namespace {

int narrow_bank_run(const sdrhip_narrow_bank* b, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                    int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t seam_block2, const float* d_state, float* d_final,
                    float* d_dc_state, void* d_ws, size_t ws_bytes)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_narrow_bank_run");
    const TunerBankDesc* tb = b->tb;
    const int K = (int)tb->ch.size();
    const FirDesc* d1 = &tb->ch[0]->fir;
    const FirDesc* d2 = b->d2;
    const bool dc = b->dc_block != 0, fm = b->form == NARROW_FM;
    // every refusal of the composed calls and of the fused launch, found here before any of them runs: a refused run has written nothing
    SDRHIP_REQUIRE(k_begin >= 0 && k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, "sdrhip_narrow_bank_run");
    SDRHIP_REQUIRE(seam_block <= 0 || seam_block >= d1->Lp, "sdrhip_narrow_bank_run: seam_block shorter than the first filter (Filter.hs:586)");
    SDRHIP_REQUIRE(seam_block2 == 0 || seam_block2 >= d2->Lp,
                   "sdrhip_narrow_bank_run: seam_block2 is 0 or at least the second filter's prepared length (Filter.hs:586)");
    const int64_t count = k_end - k_begin;
    SDRHIP_REQUIRE(K == 1 || out_stride >= count, "sdrhip_narrow_bank_run: a channel's row holds its outputs");
    SDRHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 3) == 0, "sdrhip_narrow_bank_run: d_out at an address that is no multiple of 4");
    SDRHIP_REQUIRE(fm || (d_state == nullptr && d_final == nullptr), "sdrhip_narrow_bank_run: d_state and d_final belong to the fmDemod form");
    SDRHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_state) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_final) & 3) == 0,
                   "sdrhip_narrow_bank_run: state arrays are floats");
    const BankForm pair{BankForm::PHASE, d_state, d_final};
    SDRHIP_REQUIRE(!pair.state_overlaps(K),
                   "sdrhip_narrow_bank_run: d_state and d_final overlap (the launch's first tile reads one while its last writes the other)");
    SDRHIP_REQUIRE(dc ? d_dc_state != nullptr : d_dc_state == nullptr,
                   "sdrhip_narrow_bank_run: d_dc_state is 2 K device floats with dc_block and NULL without");
    SDRHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_dc_state) & 3) == 0, "sdrhip_narrow_bank_run: the dc state is floats");
    if (count == 0) {
        // as sdrhip_fm_demod_run_rows over an empty range: d_final = d_state (or zeros), on every route; the dc state stays
        if (fm && d_final != nullptr) {
            launch_fm_demod_rows(s, K, nullptr, 0, nullptr, 0, 0, false, d_state, d_final);
            SDRHIP_CHECK_HIP(hipGetLastError());
        }
        return SDRHIP_OK;
    }
    SDRHIP_REQUIRE(count_ok(b, count), "sdrhip_narrow_bank_run: the stage-1 range of the run has 2^31 - 1 outputs or more");
    const int64_t j_begin = k_begin * d2->factor, n1 = stage1_count(d2, count), j_end = j_begin + n1;
    SDRHIP_REQUIRE(j_begin * d1->factor >= in_base, "sdrhip_narrow_bank_run: first window starts before d_in");
    SDRHIP_REQUIRE(d_in != nullptr && d_out != nullptr, "sdrhip_narrow_bank_run");
    SDRHIP_REQUIRE(fmt != IN_I16 || (reinterpret_cast<uintptr_t>(d_in) & 3) == 0,
                   "sdrhip_narrow_bank_run: int16 IQ at an address that is no multiple of 4");
    const int64_t np1 = row_floats(n1);
    float* ws = static_cast<float*>(d_ws);
    SDRHIP_REQUIRE(d_ws != nullptr && (reinterpret_cast<uintptr_t>(d_ws) & 15) == 0,
                   "sdrhip_narrow_bank_run: a 16-byte aligned workspace of sdrhip_narrow_bank_workspace_bytes(b, count)");
    const Geom g2 = bank_geom(d2, j_begin, k_begin, k_end, seam_block2);
    const int route = b->route;
    const bool fits = narrow_rows_fits(g2, d2->corder, K, ws, 2 * np1);
    if (route == 1 && !fits) {
        set_error("sdrhip_narrow_bank_run: the fused route serves a second decimator in the AVX order with a factor of at most 16, up to 128 "
                  "prepared taps and seam_block2 equal to 0 or in [numCoeffs, 2^30); this run is none of that (route 0 or 2 runs it)");
        return SDRHIP_ERR_ARG;
    }
    const bool fused = fits && (route == 1 || (route == 0 && narrow_bank_auto(K, b->form, dc, d2->factor, d2->Lp, seam_block2, count)));
    // route 0 may fall back, so it asks for what route 2 asks for
    const size_t need = route == 1 ? route1_bytes(b, K, count) : route2_bytes(b, K, count);
    SDRHIP_REQUIRE(ws_bytes >= need, "sdrhip_narrow_bank_run: a workspace of sdrhip_narrow_bank_workspace_bytes(b, count)");

    float* iq1 = ws;
    // the one step of the fused route that can fail for a reason of its own comes before any launch (the Pipe makes the same call)
    int rc;
    if (fused && (rc = d2->ensure_device()) != SDRHIP_OK) return rc;
    // the first launch of either route: whatever the tuner bank refuses on its own route setting, it refuses before any device work
    if ((rc = tuner_bank_run(tb, s, d_in, fmt, in_base, iq1, 2 * np1, j_begin, j_end, seam_block)) != SDRHIP_OK) return rc;
    float* rest = iq1 + (size_t)K * 2 * (size_t)np1;
    return narrow_stage2(b, s, fused, iq1, 2 * np1, j_begin, n1, d_out, out_stride, k_begin, k_end, seam_block2, d_state, d_final, d_dc_state,
                         rest, ws_bytes - (size_t)(rest - ws) * sizeof(float));
}

}  // namespace
}  // namespace sdrhip

using namespace sdrhip;

static_assert(SDRHIP_NARROW_ENV == NARROW_ENV && SDRHIP_NARROW_FM == NARROW_FM, "the header's forms are the kernel's");

extern "C" {

int sdrhip_narrow_bank_create(sdrhip_narrow_bank** b, const sdrhip_tuner_bank* tuner_bank, const sdrhip_decimator* decimator2, int form,
                              int dc_block)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_narrow_bank_create");
    *b = nullptr;
    SDRHIP_REQUIRE(tuner_bank != nullptr, "sdrhip_narrow_bank_create: a tuner bank");
    SDRHIP_REQUIRE(decimator2 != nullptr, "sdrhip_narrow_bank_create: a second decimator");
    SDRHIP_REQUIRE(decimator2->cplx, "sdrhip_narrow_bank_create: the second decimator works on complex data");
    SDRHIP_REQUIRE(form == SDRHIP_NARROW_ENV || form == SDRHIP_NARROW_FM, "sdrhip_narrow_bank_create: form is SDRHIP_NARROW_ENV or SDRHIP_NARROW_FM");
    SDRHIP_REQUIRE(dc_block == 0 || dc_block == 1, "sdrhip_narrow_bank_create: dc_block is 0 or 1");
    SDRHIP_REQUIRE(dc_block == 0 || form == SDRHIP_NARROW_ENV, "sdrhip_narrow_bank_create: dcBlocker follows the envelope form only");
    sdrhip_narrow_bank* a = new sdrhip_narrow_bank();
    a->tb = tuner_bank;
    a->d2 = decimator2;
    a->form = form;
    a->dc_block = dc_block;
    *b = a;
    return SDRHIP_OK;
}

void sdrhip_narrow_bank_destroy(sdrhip_narrow_bank* b) { delete b; }

int sdrhip_narrow_bank_channels(const sdrhip_narrow_bank* b) { return b ? (int)b->tb->ch.size() : SDRHIP_ERR_ARG; }

int sdrhip_narrow_bank_set_route(sdrhip_narrow_bank* b, int route)
{
    SDRHIP_REQUIRE(b != nullptr && route >= 0 && route <= 2, "sdrhip_narrow_bank_set_route");
    b->route = route;
    return SDRHIP_OK;
}

size_t sdrhip_narrow_bank_workspace_bytes(const sdrhip_narrow_bank* b, int64_t count)
{
    if (b == nullptr || !count_ok(b, count)) return 0;
    const int K = (int)b->tb->ch.size();
    return b->route == 1 ? route1_bytes(b, K, count) : route2_bytes(b, K, count);
}

int sdrhip_narrow_bank_stage1_range(const sdrhip_narrow_bank* b, int64_t k_begin, int64_t k_end, int64_t* j_begin, int64_t* j_end)
{
    SDRHIP_REQUIRE(b != nullptr && j_begin != nullptr && j_end != nullptr, "sdrhip_narrow_bank_stage1_range");
    SDRHIP_REQUIRE(k_begin >= 0 && k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, "sdrhip_narrow_bank_stage1_range");
    *j_begin = k_begin * b->d2->factor;
    *j_end = k_end == k_begin ? *j_begin : *j_begin + stage1_count(b->d2, k_end - k_begin);
    return SDRHIP_OK;
}

int sdrhip_narrow_bank_run(const sdrhip_narrow_bank* b, void* stream, const float* d_in, int64_t in_base, float* d_out, int64_t out_stride,
                           int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t seam_block2, const float* d_state, float* d_final,
                           float* d_dc_state, void* d_workspace, size_t workspace_bytes)
{
    return narrow_bank_run(b, (hipStream_t)stream, d_in, IN_CF32, in_base, d_out, out_stride, k_begin, k_end, seam_block, seam_block2, d_state,
                           d_final, d_dc_state, d_workspace, workspace_bytes);
}
int sdrhip_narrow_bank_run_u8(const sdrhip_narrow_bank* b, void* stream, const uint8_t* d_in_iq, int64_t in_base, float* d_out,
                              int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t seam_block2,
                              const float* d_state, float* d_final, float* d_dc_state, void* d_workspace, size_t workspace_bytes)
{
    return narrow_bank_run(b, (hipStream_t)stream, d_in_iq, IN_U8, in_base, d_out, out_stride, k_begin, k_end, seam_block, seam_block2, d_state,
                           d_final, d_dc_state, d_workspace, workspace_bytes);
}
int sdrhip_narrow_bank_run_i16(const sdrhip_narrow_bank* b, void* stream, const int16_t* d_in_iq, int64_t in_base, float* d_out,
                               int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t seam_block2,
                               const float* d_state, float* d_final, float* d_dc_state, void* d_workspace, size_t workspace_bytes)
{
    return narrow_bank_run(b, (hipStream_t)stream, d_in_iq, IN_I16, in_base, d_out, out_stride, k_begin, k_end, seam_block, seam_block2, d_state,
                           d_final, d_dc_state, d_workspace, workspace_bytes);
}

long long sdrhip_debug_narrow_bank_launches(void) { return narrow_bank_launch_count(); }
int sdrhip_debug_narrow_bank_tile(int form) { return form == SDRHIP_NARROW_ENV || form == SDRHIP_NARROW_FM ? narrow_tile_advance(form) : 0; }

}  // extern "C"
