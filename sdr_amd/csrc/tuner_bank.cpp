// tuner_bank.cpp -- the tuner bank of include/sdr_hip.h: descriptor, routes and the auto rule (kernels: kernels_tuner_bank.hip).
//
// Routes.  Banked: ONE launch of the tuner's fused tile kernel with a channel axis (and one fix-up launch for all channels where the
// tuner's fused route takes one), wherever that route fits a launch (tuner_fused_fits: AVX order, decimation 4 / 8 / 16, up to 128
// prepared taps, seam_block >= 0, aligned tile starts).  Channel by channel: tuner_run of the bank's own K tuner descriptors one after
// the other on the caller's stream -- the tuner's fused / two-pass logic, unchanged; every order, factor and alignment.
#include <math.h>

#include <mutex>
#include <string>

#include "descriptors.hpp"

namespace sdrhip {

static_assert(SDRHIP_TUNER_BANK_MAX_CHANNELS == kTunerBankMaxChannels, "the header's limit is the kernel's");

// auto, read from tools/tuner_bank_bench.py (profiles/tuner_bank_bench.txt) with the FM bank's rule: a point is banked where the
// banked launch's SLOWEST round was below the K tuner runs' FASTEST.  The sweep is a rectangle -- 1 / 2 / 4 / 8 / 12 / 32 channels x
// launches of 8192, 2^17, 2^20 and 2^24 input samples of the 128-tap / 8 shape, u8 and cfloat -- and at EVERY point of it with K >= 2 the
// banked launch is ahead by that rule, for both input types (0.53 .. 0.03 of the K runs' time at one block, 0.92 .. 0.73 at 2^24
// samples): no crossover was found, so the bounds are the rectangle's edges.  One channel is one launch either way and NOT level for
// cfloat input (8.1 against 7.6 us at one block, 37.0 against 35.1 at 2^24 samples): one channel goes to its tuner.  Everything outside
// the rectangle -- more than 2^24 samples per launch -- goes channel by channel.  The bound is in INPUT SAMPLES of the launch,
// count * factor: a launch of the other factors or of fewer taps reads the same samples with no more arithmetic per sample than the
// measured shape, and a launch shorter than one block is no less launch-bound than one block, so neither is held to be outside.
//
// int16 input, read from `tools/tuner_bank_bench.py --i16` (profiles/tuner_i16_bench.txt) by the same criterion over the same
// rectangle: at EVERY point with K >= 2 the banked int16 launch's slowest round is below the K run_i16 calls' fastest (0.52 .. 0.03 of
// their time at one block, 0.90 .. 0.78 at 2^24 samples), so the sweep confirms the u8 / cfloat rectangle and the bounds are again its
// edges, not crossovers; nothing beyond 2^24 samples per launch is measured and the rule is not widened.  One channel goes to its tuner,
// which for int16 launches the same kernel with one channel: level by construction, and measured so (0.995 .. 1.001).
static const int kBankAutoMinChannels = 2;
static const int64_t kBankAutoMaxSamples = (int64_t)1 << 24;

static bool bank_auto(int channels, int64_t samples)
{
    return channels >= kBankAutoMinChannels && samples <= kBankAutoMaxSamples;
}

static std::mutex g_bank_upload_mu;

TunerBankDesc::~TunerBankDesc()
{
    for (TunerDesc* t : ch) delete t;
    if (d_tables) (void)hipFree(d_tables);
}

int TunerBankDesc::ensure_device() const
{
    int rc = ch[0]->fir.ensure_device();       // also refuses a device other than the one of the first use
    if (rc != SDRHIP_OK) return rc;
    std::lock_guard<std::mutex> lk(g_bank_upload_mu);
    if (d_tables) return SDRHIP_OK;
    return upload_floats(&d_tables, h_tables);
}

int tuner_bank_run(const TunerBankDesc* b, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                   int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_tuner_bank_run");
    const int K = (int)b->ch.size();
    const FirDesc* d = &b->ch[0]->fir;         // ranges and taps are the same for every channel
    // what sdrhip_tuner_run refuses, found for the whole bank before any channel runs: a refused run has written no row
    SDRHIP_REQUIRE(k_begin >= 0 && k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, "sdrhip_tuner_bank_run");
    SDRHIP_REQUIRE(k_begin * d->factor >= in_base, "sdrhip_tuner_bank_run: first window starts before d_in");
    SDRHIP_REQUIRE(seam_block <= 0 || seam_block >= d->Lp, "sdrhip_tuner_bank_run: seam block shorter than the filter (Filter.hs:586)");
    SDRHIP_REQUIRE((out_stride & 1) == 0, "sdrhip_tuner_bank_run: an odd out_stride (rows stay 8-byte aligned)");
    SDRHIP_REQUIRE(K == 1 || out_stride >= 2 * (k_end - k_begin), "sdrhip_tuner_bank_run: a channel's row holds its outputs");
    if (k_end == k_begin) return SDRHIP_OK;
    SDRHIP_REQUIRE(d_in != nullptr && d_out != nullptr, "sdrhip_tuner_bank_run");
    SDRHIP_REQUIRE(fmt != IN_I16 || (reinterpret_cast<uintptr_t>(d_in) & 3) == 0,
                   "sdrhip_tuner_bank_run: int16 IQ at an address that is no multiple of 4");
    const Geom g = bank_geom(d, in_base, k_begin, k_end, seam_block);
    const int route = b->route;
    const bool fits = bank_fused_fits(b, g, d_in, fmt, BankForm{}, d_out);
    if (route == 1 && !fits) {
        set_error("sdrhip_tuner_bank_run: the banked launch serves the AVX order, factors 4 / 8 / 16, up to 128 prepared taps, seam_block >= 0 "
                  "and a 16-byte aligned first window; this launch is none of that (route 0 or 2 runs it)");
        return SDRHIP_ERR_ARG;
    }
    if (fits && (route == 1 || (route == 0 && bank_auto(K, (int64_t)g.count * g.D)))) {
        int rc = bank_fused(b, s, g, d_in, fmt, BankForm{}, d_out, out_stride);
        if (rc != kBankNotThisShape) return rc;
        if (route == 1) {
            set_error("sdrhip_tuner_bank_run: the banked launch refused a launch its predicate admitted");
            return SDRHIP_ERR_ARG;
        }
    }
    for (int j = 0; j < K; j++) {
        int rc = tuner_run(b->ch[j], s, d_in, fmt, in_base, d_out + (int64_t)j * out_stride, k_begin, k_end, seam_block);
        if (rc != SDRHIP_OK) return rc;
    }
    return SDRHIP_OK;
}

// ---- the output forms (descriptors.hpp: BankForm) -----------------------------------------------------------------------------------
bool BankForm::state_overlaps(int channels) const
{
    if (kind != PHASE || d_state == nullptr || d_final == nullptr) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(d_state), y = reinterpret_cast<uintptr_t>(d_final), n = (uintptr_t)channels * 2 * sizeof(float);
    return x < y + n && y < x + n;
}

Geom bank_geom(const FirDesc* d, int64_t in_base, int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    Geom g;
    g.in_base = in_base;
    g.k_begin = k_begin;
    g.count = (int)(k_end - k_begin);
    g.I = 1;
    g.D = d->factor;
    g.Lp = d->Lp;
    g.seamBI = seam_block;
    return g;
}

// Where the banked launch fits: the tuner's fused route (the Cross taps are the prepared plain taps, on the device once the descriptor
// is), the alignment of complex rows for the form that has them, and for the phase form an in-tile seam test that works in 32 bits.
// The bank objects, the Pipes and bank_fused all ask here.  launch_bank<OUT> (kernels_tuner_bank.hip) additionally refuses channel
// counts and periods that the create calls exclude, and strides and float-row addresses that every caller has checked or made itself.
bool bank_fused_fits(const TunerBankDesc* tb, const Geom& g, const void* d_in, InFmt fmt, const BankForm& form, const float* d_out)
{
    const FirDesc* d = &tb->ch[0]->fir;
    if (form.kind == BankForm::PHASE && g.seamBI >= ((int64_t)1 << 30)) return false;
    return d->corder == CO_L4 && tuner_fused_fits(g, d->Lp, true, d_in, fmt, form.kind == BankForm::IQ ? d_out : nullptr, 1);
}

int bank_fused(const TunerBankDesc* tb, hipStream_t s, const Geom& g, const void* d_in, InFmt fmt, const BankForm& form, float* d_out,
               int64_t out_stride)
{
    int rc = tb->ensure_device();
    if (rc != SDRHIP_OK) return rc;
    const FirDesc* d = &tb->ch[0]->fir;
    const int K = (int)tb->ch.size();
    bool launched;
    switch (form.kind) {
    case BankForm::IQ:
        launched = launch_tuner_bank(s, g, d->d_plain, d->Lp, d->d_cross, d_in, fmt, d_out, out_stride, tb->d_tables, K, tb->off, tb->period, true);
        break;
    case BankForm::ENV:
        launched = launch_am_bank(s, g, d->d_plain, d->Lp, d->d_cross, d_in, fmt, d_out, out_stride, tb->d_tables, K, tb->off, tb->period);
        break;
    default:
        launched = launch_nfm_bank(s, g, d->d_plain, d->Lp, d->d_cross, d_in, fmt, d_out, out_stride, tb->d_tables, K, tb->off, tb->period,
                                   form.d_state, form.d_final);
    }
    if (!launched) return kBankNotThisShape;
    SDRHIP_CHECK_HIP(hipGetLastError());
    return SDRHIP_OK;
}

int bank_composed(const TunerBankDesc* tb, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                  int64_t k_begin, int64_t k_end, int64_t seam_block, const BankForm& form, float* d_iq)
{
    const int K = (int)tb->ch.size();
    const int64_t np = row_floats(k_end - k_begin);
    // (tuner_bank_run is what sdrhip_tuner_bank_run / _run_u8 / _run_i16 call with their input type)
    int rc = tuner_bank_run(tb, s, d_in, fmt, in_base, d_iq, 2 * np, k_begin, k_end, seam_block);
    if (rc != SDRHIP_OK) return rc;
    if (form.kind == BankForm::ENV) return sdrhip_am_demod_run_rows(s, d_iq, 2 * np, d_out, out_stride, K, k_end - k_begin);
    return sdrhip_fm_demod_run_rows(s, d_iq, 2 * np, k_begin, d_out, out_stride, K, k_begin, k_end, form.d_state, form.d_final);
}

// Outputs [k_begin, k_end) of every channel, all Cross, in ONE launch (kernels_tuner_bank.hip: k_tuner_bank_cross): what
// tuner_bank_run(..., seam_block = -1) computes channel by channel, for the banks' Pipes (pipes.cpp) and nobody else -- the routes and
// the auto rules of the bank objects are not involved.
int bank_cross(const TunerBankDesc* tb, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
               int64_t k_begin, int64_t k_end, const BankForm& form)
{
    SDRHIP_REQUIRE(tb != nullptr && d_in != nullptr && d_out != nullptr, "bank_cross");
    const FirDesc* d = &tb->ch[0]->fir;
    const int K = (int)tb->ch.size();
    SDRHIP_REQUIRE(k_begin >= 0 && k_end > k_begin && k_end - k_begin < (int64_t)0x7fffffff, "bank_cross");
    SDRHIP_REQUIRE(k_begin * d->factor >= in_base, "bank_cross: first window starts before d_in");
    SDRHIP_REQUIRE(!form.state_overlaps(K), "bank_cross: d_state and d_final overlap");
    int rc = tb->ensure_device();
    if (rc != SDRHIP_OK) return rc;
    const Geom g = bank_geom(d, in_base, k_begin, k_end, -1);
    bool launched;
    switch (form.kind) {
    case BankForm::IQ: launched = launch_tuner_bank_cross(s, g, d->d_cross, d_in, fmt, d_out, out_stride, tb->d_tables, K, tb->off, tb->period); break;
    case BankForm::ENV: launched = launch_am_bank_cross(s, g, d->d_cross, d_in, fmt, d_out, out_stride, tb->d_tables, K, tb->off, tb->period); break;
    default:
        launched = launch_nfm_bank_cross(s, g, d->d_cross, d_in, fmt, d_out, out_stride, tb->d_tables, K, tb->off, tb->period, form.d_state,
                                         form.d_final);
    }
    if (!launched) {
        set_error("bank_cross: the all-Cross launch refused its channels, stride or pointers");
        return SDRHIP_ERR_ARG;
    }
    SDRHIP_CHECK_HIP(hipGetLastError());
    return SDRHIP_OK;
}

int bank_form_run(const TunerBankDesc* tb, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t out_stride,
                  int64_t k_begin, int64_t k_end, int64_t seam_block, const BankForm& form, float* d_iq)
{
    SDRHIP_REQUIRE(form.kind != BankForm::IQ && k_begin >= 0 && k_end > k_begin && !form.state_overlaps((int)tb->ch.size()), "bank_form_run");
    const Geom g = bank_geom(&tb->ch[0]->fir, in_base, k_begin, k_end, seam_block);
    if (bank_fused_fits(tb, g, d_in, fmt, form, d_out)) {
        int rc = bank_fused(tb, s, g, d_in, fmt, form, d_out, out_stride);
        if (rc != kBankNotThisShape) return rc;
    }
    SDRHIP_REQUIRE(d_iq != nullptr, "bank_form_run: no scratch for the composed route");
    return bank_composed(tb, s, d_in, fmt, in_base, d_out, out_stride, k_begin, k_end, seam_block, form, d_iq);
}

}  // namespace sdrhip

using namespace sdrhip;

extern "C" {

int sdrhip_tuner_bank_create(sdrhip_tuner_bank** b, int order, int factor, const float* coeffs, int ncoeffs, int channels,
                             const float* const* osc_iq, const int* periods)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_tuner_bank_create");
    *b = nullptr;
    SDRHIP_REQUIRE(channels >= 1 && channels <= SDRHIP_TUNER_BANK_MAX_CHANNELS, "sdrhip_tuner_bank_create: 1 .. 32 channels");
    SDRHIP_REQUIRE(osc_iq != nullptr && periods != nullptr, "sdrhip_tuner_bank_create");
    for (int j = 0; j < channels; j++) {
        SDRHIP_REQUIRE(osc_iq[j] != nullptr, "sdrhip_tuner_bank_create: every channel has a table (a channel on the centre: {1, 0})");
        SDRHIP_REQUIRE(periods[j] >= 1 && periods[j] <= 65536, "sdrhip_tuner_bank_create: period 1 .. 65536");
        for (size_t i = 0; i < 2 * (size_t)periods[j]; i++)
            SDRHIP_REQUIRE(isfinite(osc_iq[j][i]), "sdrhip_tuner_bank_create: non-finite table entry");
    }
    sdrhip_tuner_bank* bk = new sdrhip_tuner_bank();
    size_t pairs = 0;
    for (int j = 0; j < channels; j++) {
        // as sdrhip_tuner_create(order, factor, coeffs, ncoeffs, osc_iq[j], periods[j])
        TunerDesc* t = new TunerDesc();
        bk->ch.push_back(t);
        int rc = fir_create(&t->fir, order, true, factor, coeffs, ncoeffs);
        if (rc != SDRHIP_OK) {
            const std::string why = get_error();                // the decimator's refusal, under this function's name
            set_error("sdrhip_tuner_bank_create: %s", why.c_str());
            delete bk;
            return rc;
        }
        t->period = periods[j];
        t->h_osc.assign(osc_iq[j], osc_iq[j] + 2 * (size_t)periods[j]);
        bk->off[j] = (int)pairs;
        bk->period[j] = periods[j];
        bk->h_tables.insert(bk->h_tables.end(), osc_iq[j], osc_iq[j] + 2 * (size_t)periods[j]);
        pairs += (size_t)periods[j];
    }
    *b = bk;
    return SDRHIP_OK;
}

void sdrhip_tuner_bank_destroy(sdrhip_tuner_bank* b) { delete b; }

int sdrhip_tuner_bank_channels(const sdrhip_tuner_bank* b) { return b ? (int)b->ch.size() : SDRHIP_ERR_ARG; }

int sdrhip_tuner_bank_period(const sdrhip_tuner_bank* b, int channel)
{
    SDRHIP_REQUIRE(b != nullptr && channel >= 0 && channel < (int)b->ch.size(), "sdrhip_tuner_bank_period");
    return b->period[channel];
}

int sdrhip_tuner_bank_num_coeffs(const sdrhip_tuner_bank* b) { return b ? b->ch[0]->fir.Lp : SDRHIP_ERR_ARG; }
int sdrhip_tuner_bank_factor(const sdrhip_tuner_bank* b) { return b ? b->ch[0]->fir.factor : SDRHIP_ERR_ARG; }

int sdrhip_tuner_bank_set_route(sdrhip_tuner_bank* b, int route)
{
    SDRHIP_REQUIRE(b != nullptr && route >= 0 && route <= 2, "sdrhip_tuner_bank_set_route");
    b->route = route;
    return SDRHIP_OK;
}

int sdrhip_tuner_bank_run(const sdrhip_tuner_bank* b, void* stream, const float* d_in, int64_t in_base, float* d_out, int64_t out_stride,
                          int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    return tuner_bank_run(b, (hipStream_t)stream, d_in, IN_CF32, in_base, d_out, out_stride, k_begin, k_end, seam_block);
}
int sdrhip_tuner_bank_run_u8(const sdrhip_tuner_bank* b, void* stream, const uint8_t* d_in_iq, int64_t in_base, float* d_out,
                             int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    return tuner_bank_run(b, (hipStream_t)stream, d_in_iq, IN_U8, in_base, d_out, out_stride, k_begin, k_end, seam_block);
}
int sdrhip_tuner_bank_run_i16(const sdrhip_tuner_bank* b, void* stream, const int16_t* d_in_iq, int64_t in_base, float* d_out,
                              int64_t out_stride, int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    return tuner_bank_run(b, (hipStream_t)stream, d_in_iq, IN_I16, in_base, d_out, out_stride, k_begin, k_end, seam_block);
}

// a banked launch is a banked launch whatever it reads
long long sdrhip_debug_tuner_bank_launches(void) { return tuner_bank_launch_count(); }
long long sdrhip_debug_tuner_bank_cross_launches(void) { return tuner_bank_cross_launch_count(); }

}  // extern "C"
