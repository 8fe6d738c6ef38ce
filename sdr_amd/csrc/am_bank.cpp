// am_bank.cpp -- the AM receiver bank of include/sdr_hip.h: every channel's envelope (and dcBlocker) from one capture.
//
// Definition (and route 2, composed): sdrhip_tuner_bank_run* into complex rows of the workspace, sdrhip_am_demod_run_rows, and with
// dc_block sdrhip_dc_blocker_run_rows from and to d_dc_state with a workspace and the default run-in -- the calls a caller makes
// without this object, through the C ABI, unchanged.
// Route 1 (fused): the tuner bank's banked launch set in the envelope form (kernels_tuner_bank.hip, OUT_ENV: the magnitude of each
// finished output is what the tile and fix-up kernels store), then the same sdrhip_dc_blocker_run_rows call.  Without dc_block the
// tile launch writes d_out and there is no workspace; with it the envelope rows pass through the workspace, because dcBlocker's row
// form refuses d_in == d_out.  Nothing is argued anew: the complex value under the magnitude is the banked launch's, the magnitude is
// kernels_am.hip's device function (am.hpp), dcBlocker is called with the same rows, length, state and run-in on both routes.
#include "descriptors.hpp"

namespace sdrhip {
namespace {

// auto, read from tools/am_bank_bench.py (profiles/am_bank_bench.txt) by the project's criterion: route 1 where its SLOWEST of 7 rounds
// was below route 2's FASTEST.  The sweep is a rectangle -- 1 / 2 / 8 / 32 channels x launches of 8192, 2^17, 2^20 and 2^24 input samples of
// the 128-tap / 8 shape, u8 / cfloat / int16, dc_block off and on -- and the three input types agree on where route 1 is ahead:
//   dc_block = 0: at all 48 points (0.75 .. 0.91 of route 2's time: the am_demod launch and the complex rows' traffic are gone), one
//     channel included (8.3 against 9.9 us at 8192 samples of u8, 33.3 against 37.8 at 2^24);
//   dc_block = 1: at all 24 points with 8 and 32 channels (0.97 .. 0.98 at 8192 samples, 0.89 at 2^17, 0.99 at 2^20, 0.94 .. 0.99 at 2^24:
//     dcBlocker's walk is most of either route, 76.9 against 79.3 us at 8192 samples x 8), and NOT at 8192 and 2^17 samples with 1 and 2 channels
//     (one channel at 8192 samples: 43.9 against 37.9 us u8, 41.8 against 37.5 cfloat, 44.2 against 39.6 int16 -- route 1 is BEHIND there; 2
//     channels 1.01 .. 1.03; at 2^17 the spreads overlap).  Two channels at 2^20 are ahead for int16 only: route 2.  One channel at the
//     2^20 and 2^24 launches and two channels at the 2^24 launch are ahead for every input type, by 0.5 .. 1.9 %, and the rule takes them
//     as the criterion says: one channel from the measured 2^20 launch (131057 outputs x 8 samples) up to 2^24 samples, two channels
//     from the measured 2^24 launch (2097137 x 8) up.  2 < K < 8 is not measured and stays on route 2.
// Everything outside the rectangle -- more than 2^24 samples per launch -- is route 2.  The bound is in INPUT SAMPLES of the launch,
// count * factor, as the tuner bank's; other factors and tap counts are held to it unmeasured.
const int64_t kAmBankAutoMaxSamples = (int64_t)1 << 24;
const int kAmBankAutoDcMinChannels = 8;
// the measured launches from which ONE channel and TWO channels with dcBlocker are ahead: 131057 and 2097137 outputs x 8 samples
const int64_t kAmBankAutoDcOneChannelMinSamples = (int64_t)131057 * 8;
const int64_t kAmBankAutoDcTwoChannelsMinSamples = (int64_t)2097137 * 8;

bool am_bank_auto(int channels, int64_t samples, bool dc)
{
    if (samples > kAmBankAutoMaxSamples) return false;
    if (!dc || channels >= kAmBankAutoDcMinChannels) return true;
    if (channels == 1) return samples >= kAmBankAutoDcOneChannelMinSamples;
    return channels == 2 && samples >= kAmBankAutoDcTwoChannelsMinSamples;
}

size_t route1_bytes(int K, int64_t count, bool dc)
{
    return dc ? (size_t)K * (size_t)row_floats(count) * sizeof(float) + dc_blocker_rows_workspace_bytes(K, count) : 0;
}

size_t route2_bytes(int K, int64_t count, bool dc)
{
    return (size_t)K * 2 * (size_t)row_floats(count) * sizeof(float) + route1_bytes(K, count, dc);
}

int am_bank_run(const sdrhip_am_bank* b, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                int64_t k_begin, int64_t k_end, int64_t seam_block, float* d_dc_state, void* d_ws, size_t ws_bytes)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_am_bank_run");
    const TunerBankDesc* tb = b->tb;
    const int K = (int)tb->ch.size();
    const FirDesc* d = &tb->ch[0]->fir;
    const bool dc = b->dc_block != 0;
    // every refusal of the three composed calls, found here before any of them runs: a refused run has written nothing
    SDRHIP_REQUIRE(k_begin >= 0 && k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, "sdrhip_am_bank_run");
    SDRHIP_REQUIRE(k_begin * d->factor >= in_base, "sdrhip_am_bank_run: first window starts before d_in");
    SDRHIP_REQUIRE(seam_block <= 0 || seam_block >= d->Lp, "sdrhip_am_bank_run: seam block shorter than the filter (Filter.hs:586)");
    const int64_t count = k_end - k_begin;
    SDRHIP_REQUIRE(K == 1 || out_stride >= count, "sdrhip_am_bank_run: a channel's row holds its outputs");
    SDRHIP_REQUIRE(dc ? d_dc_state != nullptr : d_dc_state == nullptr,
                   "sdrhip_am_bank_run: d_dc_state is 2 K device floats with dc_block and NULL without");
    if (count == 0) return SDRHIP_OK;
    SDRHIP_REQUIRE(d_in != nullptr && d_out != nullptr && (reinterpret_cast<uintptr_t>(d_out) & 3) == 0, "sdrhip_am_bank_run");
    SDRHIP_REQUIRE(fmt != IN_I16 || (reinterpret_cast<uintptr_t>(d_in) & 3) == 0,
                   "sdrhip_am_bank_run: int16 IQ at an address that is no multiple of 4");
    const Geom g = bank_geom(d, in_base, k_begin, k_end, seam_block);
    const BankForm form{BankForm::ENV};
    const int route = b->route;
    // where the tuner bank's banked launch fits (tuner_bank.cpp), the complex rows' alignment aside: there are none
    const bool fits = bank_fused_fits(tb, g, d_in, fmt, form, nullptr);
    if (route == 1 && !fits) {
        set_error("sdrhip_am_bank_run: the fused route serves what the tuner bank's banked launch serves -- the AVX order, factors 4 / 8 / 16, "
                  "up to 128 prepared taps, seam_block >= 0 and a 16-byte aligned first window; this launch is none of that (route 0 or 2 runs it)");
        return SDRHIP_ERR_ARG;
    }
    const bool fused = fits && (route == 1 || (route == 0 && am_bank_auto(K, count * g.D, dc)));
    // route 0 may fall back, so it asks for what route 2 asks for
    const size_t need = route == 1 ? route1_bytes(K, count, dc) : route2_bytes(K, count, dc);
    SDRHIP_REQUIRE(need == 0 || (d_ws != nullptr && ws_bytes >= need && (reinterpret_cast<uintptr_t>(d_ws) & 15) == 0),
                   "sdrhip_am_bank_run: a 16-byte aligned workspace of sdrhip_am_bank_workspace_bytes(b, count)");

    const int64_t np = row_floats(count);
    // workspace: [complex rows (composed) | envelope rows (dc_block) | dcBlocker's own]; without dc_block the envelope rows are d_out's
    auto run = [&](float* iq, float* ws_env) -> int {
        float* env = dc ? ws_env : d_out;
        const int64_t env_stride = dc ? np : out_stride;
        int rc = iq == nullptr ? bank_fused(tb, s, g, d_in, fmt, form, env, env_stride)
                               : bank_composed(tb, s, d_in, fmt, in_base, env, env_stride, k_begin, k_end, seam_block, form, iq);
        if (rc != SDRHIP_OK || !dc) return rc;
        float* dcw = env + (size_t)K * (size_t)np;
        return sdrhip_dc_blocker_run_rows(s, env, np, d_out, out_stride, K, count, d_dc_state, d_dc_state, dcw,
                                          ws_bytes - (size_t)(dcw - static_cast<float*>(d_ws)) * sizeof(float), 0);
    };
    float* ws = static_cast<float*>(d_ws);
    if (fused) {
        int rc = run(nullptr, ws);
        if (rc != kBankNotThisShape) return rc;
        if (route == 1) {
            set_error("sdrhip_am_bank_run: the envelope launch refused a launch its predicate admitted");
            return SDRHIP_ERR_ARG;
        }
        // auto: nothing was launched and the composed route runs it (its workspace was asked for above), as the tuner bank falls through
    }
    return run(ws, ws + (size_t)K * 2 * (size_t)np);
}

}  // namespace
}  // namespace sdrhip

using namespace sdrhip;

extern "C" {

int sdrhip_am_bank_create(sdrhip_am_bank** b, const sdrhip_tuner_bank* tuner_bank, int dc_block)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_am_bank_create");
    *b = nullptr;
    SDRHIP_REQUIRE(tuner_bank != nullptr, "sdrhip_am_bank_create: a tuner bank");
    SDRHIP_REQUIRE(dc_block == 0 || dc_block == 1, "sdrhip_am_bank_create: dc_block is 0 or 1");
    sdrhip_am_bank* a = new sdrhip_am_bank();
    a->tb = tuner_bank;
    a->dc_block = dc_block;
    *b = a;
    return SDRHIP_OK;
}

void sdrhip_am_bank_destroy(sdrhip_am_bank* b) { delete b; }

int sdrhip_am_bank_channels(const sdrhip_am_bank* b) { return b ? (int)b->tb->ch.size() : SDRHIP_ERR_ARG; }

int sdrhip_am_bank_set_route(sdrhip_am_bank* b, int route)
{
    SDRHIP_REQUIRE(b != nullptr && route >= 0 && route <= 2, "sdrhip_am_bank_set_route");
    b->route = route;
    return SDRHIP_OK;
}

size_t sdrhip_am_bank_workspace_bytes(const sdrhip_am_bank* b, int64_t count)
{
    if (b == nullptr || count <= 0 || count >= (int64_t)0x7fffffff) return 0;
    return route2_bytes((int)b->tb->ch.size(), count, b->dc_block != 0);
}

int sdrhip_am_bank_run(const sdrhip_am_bank* b, void* stream, const float* d_in, int64_t in_base, float* d_out, int64_t out_stride,
                       int64_t k_begin, int64_t k_end, int64_t seam_block, float* d_dc_state, void* d_workspace, size_t workspace_bytes)
{
    return am_bank_run(b, (hipStream_t)stream, d_in, IN_CF32, in_base, d_out, out_stride, k_begin, k_end, seam_block, d_dc_state,
                       d_workspace, workspace_bytes);
}
int sdrhip_am_bank_run_u8(const sdrhip_am_bank* b, void* stream, const uint8_t* d_in_iq, int64_t in_base, float* d_out, int64_t out_stride,
                          int64_t k_begin, int64_t k_end, int64_t seam_block, float* d_dc_state, void* d_workspace, size_t workspace_bytes)
{
    return am_bank_run(b, (hipStream_t)stream, d_in_iq, IN_U8, in_base, d_out, out_stride, k_begin, k_end, seam_block, d_dc_state,
                       d_workspace, workspace_bytes);
}
int sdrhip_am_bank_run_i16(const sdrhip_am_bank* b, void* stream, const int16_t* d_in_iq, int64_t in_base, float* d_out, int64_t out_stride,
                           int64_t k_begin, int64_t k_end, int64_t seam_block, float* d_dc_state, void* d_workspace, size_t workspace_bytes)
{
    return am_bank_run(b, (hipStream_t)stream, d_in_iq, IN_I16, in_base, d_out, out_stride, k_begin, k_end, seam_block, d_dc_state,
                       d_workspace, workspace_bytes);
}

long long sdrhip_debug_am_bank_launches(void) { return am_bank_launch_count(); }
long long sdrhip_debug_am_bank_fixup_launches(void) { return am_bank_fixup_launch_count(); }
long long sdrhip_debug_am_bank_cross_launches(void) { return am_bank_cross_launch_count(); }

}  // extern "C"
