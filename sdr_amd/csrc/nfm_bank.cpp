// nfm_bank.cpp -- the narrow-band FM demodulator bank of include/sdr_hip.h: fmDemod of every channel of one capture.
//
// Definition (and route 2, composed): sdrhip_tuner_bank_run* into complex rows of the workspace, then sdrhip_fm_demod_run_rows with
// d_last_iq = d_state and d_last_out = d_final -- the calls a caller makes without this object, through the C ABI, unchanged.
// Route 1 (fused): the tuner bank's tile launch in the fmDemod form (kernels_tuner_bank.hip, OUT_FM) and nothing else: ONE launch, no
// workspace.  A finished output y[k] is stored as fm_phase(y[k], y[k - 1]); the predecessor comes from the neighbouring thread, from
// the overlapped pair of a tile's thread 0, or -- for the launch's first output -- from d_state.  Every Cross output is computed in
// the tile (a fix-up launch could not repair the two phase differences a Cross output takes part in).  Nothing is argued anew: the
// complex value under the phase is the banked launch's, the phase is demod.hpp's device function, as fmDemod's rows form.
#include "descriptors.hpp"

namespace sdrhip {
namespace {

// auto, read from tools/nfm_bank_bench.py (profiles/nfm_bank_bench.txt) by the project's criterion: route 1 where its SLOWEST of 7 rounds
// was below route 2's FASTEST, for ALL THREE input types (they agree but for a few points, named below).  The sweep: 1 / 2 / 8 / 32
// channels x launches of 8192, 2^17, 2^20 and 2^24 input samples of the 128-tap shape, u8 / cfloat / int16, factors 8 and 16, seam_block
// 0 and 8192.  With n = (k_end - k_begin - 1) * factor + numCoeffs the input samples of the launch, route 1 is ahead (us per run, u8):
//   factor 8,  seam 0:     at all 48 points (0.63 .. 0.97 of route 2's time: 10.0 against 11.2 us for one channel at 8192 samples,
//                          977 against 1045 us for 32 channels at 2^24)                                         -> n <= 2^24, any K
//   factor 8,  seam 8192:  at every point up to 2^20 (0.72 .. 0.96) and at 2^24 with ONE channel (0.79 .. 0.86); NOT at 2^24 with 2, 8
//                          and 32 channels (u8 1.06 / 1.31 / 1.09, cfloat and int16 1.06 .. 1.07 at 8 channels: every output of such a
//                          launch pays the in-tile seam test's modulo, and its 2048 seams' Cross outputs are recomputed by whole tiles'
//                          waves where route 2's fix-up launch takes one thread each)              -> K == 1: n <= 2^24; else n <= 2^20
//   factor 16, seam 0:     1 and 2 channels at all sizes (0.64 .. 0.96); 8 channels up to 2^17 (2^20: cfloat 1.04; 2^24: 1.03 / 1.04);
//                          32 channels at 8192 only (2^17: cfloat 1.11; 2^24: 1.01 / 1.04; the 2^20 point between them is ahead by 1 .. 2 %
//                          and is left on route 2)                 -> K <= 2: n <= 2^24; K == 8: n <= 2^17; K == 32: n <= 8192
//   factor 16, seam 8192:  NOT at 8192 samples, whatever K (1.07 .. 1.14: 19.6 against 18.0 us -- one block, whose tile holds the
//                          whole launch and computes Cross outputs beside it); at 2^17 for every K (0.43 .. 0.77), at 2^20 for 1, 2 and 8
//                          channels (0.41 .. 0.78; 32 channels 1.09 .. 1.20), at 2^24 for one channel only (0.91 .. 0.99; 2 / 8 / 32
//                          channels 1.01 .. 1.49)      -> K == 1: 2^17 <= n <= 2^24; K == 2, 8: 2^17 <= n <= 2^20; K == 32: n == 2^17 .. 2^17
// A channel count between two measured ones is fused only where BOTH neighbours are.  seam_block 0 takes the seam-0 rows; seam_block
// >= 8192 takes the seam-8192 rows (a longer block has fewer Cross outputs: between the two measured cases, held to the slower
// unmeasured); 0 < seam_block < 8192 (more seams a tile than measured, up to every output Cross), factor 4, and everything beyond 2^24
// samples a launch are not measured and are route 2.  Other tap counts are held to the rule unmeasured.  Below 8192 samples the
// launch count decides (one against two or three), so a row that is ahead at 8192 has no lower bound.
struct AutoRange { int64_t lo, hi; };        // fused iff lo <= n <= hi; hi = 0: never
constexpr int64_t k13 = 8192, k17 = (int64_t)1 << 17, k20 = (int64_t)1 << 20, k24 = (int64_t)1 << 24;
// [factor 8 / 16][seam 0 / seamed][1, 2, 8, 32 channels]
const AutoRange kNfmAuto[2][2][4] = {
    {{{0, k24}, {0, k24}, {0, k24}, {0, k24}}, {{0, k24}, {0, k20}, {0, k20}, {0, k20}}},
    {{{0, k24}, {0, k24}, {0, k17}, {0, k13}}, {{k17, k24}, {k17, k20}, {k17, k20}, {k17, k17}}},
};
const int64_t kNfmAutoMinSeam = 8192;

bool nfm_bank_auto(int channels, int factor, int64_t seam_block, int64_t n)
{
    if (factor != 8 && factor != 16) return false;
    if (seam_block != 0 && seam_block < kNfmAutoMinSeam) return false;
    const AutoRange* row = kNfmAuto[factor == 16][seam_block != 0];
    static const int kMeasured[4] = {1, 2, 8, 32};
    for (int i = 0; i < 4; i++) {
        if (channels > kMeasured[i]) continue;
        // channels == kMeasured[i], or between kMeasured[i - 1] and it: both neighbours
        const bool here = n >= row[i].lo && n <= row[i].hi;
        if (channels == kMeasured[i] || i == 0) return here;
        return here && n >= row[i - 1].lo && n <= row[i - 1].hi;
    }
    return false;
}

size_t route2_bytes(int K, int64_t count) { return (size_t)K * 2 * (size_t)row_floats(count) * sizeof(float); }

int nfm_bank_run(const sdrhip_nfm_bank* b, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                 int64_t k_begin, int64_t k_end, int64_t seam_block, const float* d_state, float* d_final, void* d_ws, size_t ws_bytes)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_nfm_bank_run");
    const TunerBankDesc* tb = b->tb;
    const int K = (int)tb->ch.size();
    const FirDesc* d = &tb->ch[0]->fir;
    // every refusal of the two composed calls and of the fused launch, found here before either runs: a refused run has written nothing
    SDRHIP_REQUIRE(k_begin >= 0 && k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, "sdrhip_nfm_bank_run");
    SDRHIP_REQUIRE(k_begin * d->factor >= in_base, "sdrhip_nfm_bank_run: first window starts before d_in");
    SDRHIP_REQUIRE(seam_block <= 0 || seam_block >= d->Lp, "sdrhip_nfm_bank_run: seam block shorter than the filter (Filter.hs:586)");
    const int64_t count = k_end - k_begin;
    SDRHIP_REQUIRE(K == 1 || out_stride >= count, "sdrhip_nfm_bank_run: a channel's row holds its outputs");
    SDRHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 3) == 0, "sdrhip_nfm_bank_run: d_out at an address that is no multiple of 4");
    SDRHIP_REQUIRE(fmt != IN_I16 || (reinterpret_cast<uintptr_t>(d_in) & 3) == 0,
                   "sdrhip_nfm_bank_run: int16 IQ at an address that is no multiple of 4");
    SDRHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_state) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_final) & 3) == 0,
                   "sdrhip_nfm_bank_run: state arrays are floats");
    const BankForm form{BankForm::PHASE, d_state, d_final};
    SDRHIP_REQUIRE(!form.state_overlaps(K),
                   "sdrhip_nfm_bank_run: d_state and d_final overlap (the launch's first tile reads one while its last writes the other)");
    if (count == 0) {
        // as sdrhip_fm_demod_run_rows over an empty range: d_final = d_state (or zeros), on every route
        if (d_final != nullptr) {
            launch_fm_demod_rows(s, K, nullptr, 0, nullptr, 0, 0, false, d_state, d_final);
            SDRHIP_CHECK_HIP(hipGetLastError());
        }
        return SDRHIP_OK;
    }
    SDRHIP_REQUIRE(d_in != nullptr && d_out != nullptr, "sdrhip_nfm_bank_run");
    const Geom g = bank_geom(d, in_base, k_begin, k_end, seam_block);
    const int route = b->route;
    // where the tuner bank's banked launch fits (tuner_bank.cpp), the complex rows' alignment aside (there are none), and the in-tile
    // seam test works in 32 bits
    const bool fits = bank_fused_fits(tb, g, d_in, fmt, form, nullptr);
    if (route == 1 && !fits) {
        set_error("sdrhip_nfm_bank_run: the fused route serves what the tuner bank's banked launch serves -- the AVX order, factors 4 / 8 / 16, "
                  "up to 128 prepared taps, 0 <= seam_block < 2^30 and a 16-byte aligned first window; this launch is none of that (route 0 or 2 "
                  "runs it)");
        return SDRHIP_ERR_ARG;
    }
    const bool fused = fits && (route == 1 || (route == 0 && nfm_bank_auto(K, g.D, seam_block, (count - 1) * g.D + g.Lp)));
    // route 0 may fall back, so it asks for what route 2 asks for
    const size_t need = route == 1 ? 0 : route2_bytes(K, count);
    SDRHIP_REQUIRE(need == 0 || (d_ws != nullptr && ws_bytes >= need && (reinterpret_cast<uintptr_t>(d_ws) & 15) == 0),
                   "sdrhip_nfm_bank_run: a 16-byte aligned workspace of sdrhip_nfm_bank_workspace_bytes(b, count)");
    if (fused) {
        int rc = bank_fused(tb, s, g, d_in, fmt, form, d_out, out_stride);
        if (rc != kBankNotThisShape) return rc;
        if (route == 1) {
            set_error("sdrhip_nfm_bank_run: the fmDemod-form launch refused a launch its predicate admitted");
            return SDRHIP_ERR_ARG;
        }
        // auto: nothing was launched and the composed route runs it (its workspace was asked for above)
    }
    return bank_composed(tb, s, d_in, fmt, in_base, d_out, out_stride, k_begin, k_end, seam_block, form, static_cast<float*>(d_ws));
}

}  // namespace
}  // namespace sdrhip

using namespace sdrhip;

extern "C" {

int sdrhip_nfm_bank_create(sdrhip_nfm_bank** b, const sdrhip_tuner_bank* tuner_bank)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_nfm_bank_create");
    *b = nullptr;
    SDRHIP_REQUIRE(tuner_bank != nullptr, "sdrhip_nfm_bank_create: a tuner bank");
    sdrhip_nfm_bank* a = new sdrhip_nfm_bank();
    a->tb = tuner_bank;
    *b = a;
    return SDRHIP_OK;
}

void sdrhip_nfm_bank_destroy(sdrhip_nfm_bank* b) { delete b; }

int sdrhip_nfm_bank_channels(const sdrhip_nfm_bank* b) { return b ? (int)b->tb->ch.size() : SDRHIP_ERR_ARG; }

int sdrhip_nfm_bank_set_route(sdrhip_nfm_bank* b, int route)
{
    SDRHIP_REQUIRE(b != nullptr && route >= 0 && route <= 2, "sdrhip_nfm_bank_set_route");
    b->route = route;
    return SDRHIP_OK;
}

size_t sdrhip_nfm_bank_workspace_bytes(const sdrhip_nfm_bank* b, int64_t count)
{
    if (b == nullptr || count <= 0 || count >= (int64_t)0x7fffffff) return 0;
    return route2_bytes((int)b->tb->ch.size(), count);
}

int sdrhip_nfm_bank_run(const sdrhip_nfm_bank* b, void* stream, const float* d_in, int64_t in_base, float* d_out, int64_t out_stride,
                        int64_t k_begin, int64_t k_end, int64_t seam_block, const float* d_state, float* d_final, void* d_workspace,
                        size_t workspace_bytes)
{
    return nfm_bank_run(b, (hipStream_t)stream, d_in, IN_CF32, in_base, d_out, out_stride, k_begin, k_end, seam_block, d_state, d_final,
                        d_workspace, workspace_bytes);
}
int sdrhip_nfm_bank_run_u8(const sdrhip_nfm_bank* b, void* stream, const uint8_t* d_in_iq, int64_t in_base, float* d_out, int64_t out_stride,
                           int64_t k_begin, int64_t k_end, int64_t seam_block, const float* d_state, float* d_final, void* d_workspace,
                           size_t workspace_bytes)
{
    return nfm_bank_run(b, (hipStream_t)stream, d_in_iq, IN_U8, in_base, d_out, out_stride, k_begin, k_end, seam_block, d_state, d_final,
                        d_workspace, workspace_bytes);
}
int sdrhip_nfm_bank_run_i16(const sdrhip_nfm_bank* b, void* stream, const int16_t* d_in_iq, int64_t in_base, float* d_out, int64_t out_stride,
                            int64_t k_begin, int64_t k_end, int64_t seam_block, const float* d_state, float* d_final, void* d_workspace,
                            size_t workspace_bytes)
{
    return nfm_bank_run(b, (hipStream_t)stream, d_in_iq, IN_I16, in_base, d_out, out_stride, k_begin, k_end, seam_block, d_state, d_final,
                        d_workspace, workspace_bytes);
}

long long sdrhip_debug_nfm_bank_launches(void) { return nfm_bank_launch_count(); }
long long sdrhip_debug_nfm_bank_cross_launches(void) { return nfm_bank_cross_launch_count(); }

}  // extern "C"
