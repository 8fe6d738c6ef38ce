// chain.cpp -- the FM receiver chain of examples/fm/fm.hs:34-41 as one device-resident
// object:  u8 IQ -> [convert fused] -> firDecimator -> fmDemod -> firResampler ->
// firFilter(sym) -> *gain.  Every stage runs with global stream indices, so a shard
// (plus a right halo) of the stream can be processed anywhere -- on any GPU --
// and yields exactly the bits the single-stream Pipes would have produced.
//
// Index spaces:  n input samples -> k decimator outputs (window [k*D1, k*D1+P1))
//   -> y[k] = phase(d[k] * conj d[k-1]) -> m resampler outputs (inputs from
//   inOff(m) = ceil(m*D2/I2)) -> q audio outputs (window [q, q+L3)).
// Seams: all four Pipes of fm.hs run with blockSizeOut = `block` and the source
// delivers `block`-sample buffers, so each stage's input blocks are `block` long.
//
// Tuner (sdrhip_fm_chain_set_tuner): `P.map (VG.zipWith (*) osc)` between convert and firDecimator.  The decimator outputs are then,
// bit for bit, sdrhip_tuner_run_u8's (kernels_tuner.hip) and everything behind them is unchanged; the oscillator phase of a sample is
// its absolute stream index mod the period, so halos, shards, pushes and saved streams need nothing new.
//
// One run (chain_run_on): derive the stage ranges of [q0, q1) once (plan_run), check the receptive field once, pick ONE route --
// the one-kernel chain, decimator + fused tail, or the stage kernels -- and launch it.  Whether a fused kernel applies is asked
// of its predicate (kernels.hpp: fm_tail_shape_ok when the chain is created, fm_chain_small_fits / fm_tail_fused_fits per run)
// together with the mode and size rule, before anything is launched or timed; the launchers launch unconditionally.
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include <exception>
#include "descriptors.hpp"
#include "host_stream.hpp"
#include "tail_plan.hpp"

using namespace sdrhip;

// fused tail in auto mode: runs of at most this many audio outputs, i.e. up to two source blocks (measured per push, in place: fused
// 27.3 / 29.1 / 36.6 us for 1 / 2 / 4 blocks, the stage kernels on their one-launch routes 30.0 / 30.7 / 32.6 -- the single workgroup
// of a one-tile run is serial)
static const int kFusedTailAutoOutputs = 768;
// the stages of the per-stage timing, in the order of sdrhip_fm_chain_read_timing's ms_sum[] (FmChain.STAGES in lib.py): decimate
// (+ seam fix-up), fmDemod, resample, filter, fused tail (fmDemod + resample + filter + gain in one kernel), whole chain in one kernel
enum Stage { kDecimate, kFmDemod, kResample, kFilter, kFusedTail, kFusedChain, kStages };
// the whole chain as ONE kernel (kernels_small.hip) in auto mode: runs of at most this many audio outputs (~7.3 M input samples);
// measured on MI355X (tools/shard_pass_probe.py): see DESIGN.md 5 "one-kernel chain"
static const int64_t kSmallChainAutoOutputs = 159 * 1728;   // round 5 (tools/launch_sweep.py): the crossover with the stage kernels sits at ~900
                                                            // source blocks (43 us either way); the old bound of 256 blocks left runs of 384 .. 768
                                                            // blocks on the stage kernels, 1.2 .. 1.6 times slower than this kernel

struct sdrhip_fm_chain {
    FirDesc decim;     // complex, factor D1
    ResampDesc resamp; // real I2/D2
    FirDesc audio;     // symmetric real
    float gain = 1.0f;
    int64_t block = 0;
    // The fused convert + decimate kernel (k_decimate_c4) covers the AVX order, decimation 4 / 8 / 16, up to 128 (4) or 256 (8, 16) taps.  Any other
    // first stage converts the u8 IQ to cfloat in the workspace first (convert.c as its own kernel, 10 B per sample) and
    // then runs the tiled cfloat decimator -- two passes, but not the one-thread-per-output u8 fallback.
    bool fused_first_stage() const
    {
        const int D = decim.factor;
        if (!((D == 4 || D == 8 || D == 16) && decim.Lp > D && decim.Lp % 4 == 0)) return false;
        if (decim.h_scaled.empty()) return false;      // a tap too small to pre-scale by 1/128 exactly (descriptors.hpp)
        if (decim.corder == CO_L4) return decim.Lp <= (D == 4 ? 128 : 256);
        return decim.corder == CO_L2 && decim.Lp <= 128;      // the SSE order's fused instantiations (kernels_fast_orders.hip)
    }

    // fmDemod -> resampler -> audio filter (* gain) as ONE kernel (kernels_tail.hip), y and z never leaving LDS.  Measured on
    // MI355X (2^29 samples per run): 0.43-0.49 ms against 0.38 + 0.02 ms for the three stage kernels and their seam fix-ups --
    // every stage is VALU-bound, fusion saves HBM traffic that was not the limit and pays 7 % recomputed overlap; but a run
    // that fills at most one tile (a push of one to six 8192-sample source blocks) costs ONE launch of a few microseconds
    // instead of eight.  mode 0 = never, 1 = always, 2 = auto (runs of at most one tile): sdrhip_fm_chain_set_fused_tail,
    // SDRHIP_FUSED_TAIL=0/1/2.  (Rounds 2-4 also measured sub-batch pipelining of one run over two streams and "fmDemod kernel + fused
    // resampler / filter": both slower, both gone; LABNOTES.)
    int fused_tail = getenv("SDRHIP_FUSED_TAIL") ? atoi(getenv("SDRHIP_FUSED_TAIL")) : 2;
    // fmDemod in the resampler's tile loader: ON by default since round 4 (with the packed-pair resampler the pass gains 1.0 %,
    // 1.005-1.011 against 1.017-1.019 ms, alternating in one process: the pair itself is slower, 0.269 against 0.159 + 0.089 ms, but
    // 0.54 GB less traffic per pass leaves the power-capped decimator 4 % more clock)
    bool fuse_demod = getenv("SDRHIP_FUSE_DEMOD") ? atoi(getenv("SDRHIP_FUSE_DEMOD")) != 0 : true;
    // The whole chain as one kernel for launch-bound runs (kernels_small.hip): 0 = never, 1 = whenever the configuration is the
    // one it is written for, 2 = auto (runs of at most small_chain_max audio outputs): sdrhip_fm_chain_set_small_chain,
    // SDRHIP_SMALL_CHAIN=0/1/2, SDRHIP_SMALL_CHAIN_MAX=<outputs>, SDRHIP_SMALL_CHAIN_TILE=<audio outputs per workgroup, 0 = by size>.
    int small_chain = getenv("SDRHIP_SMALL_CHAIN") ? atoi(getenv("SDRHIP_SMALL_CHAIN")) : 2;
    int64_t small_chain_max = getenv("SDRHIP_SMALL_CHAIN_MAX") ? atoll(getenv("SDRHIP_SMALL_CHAIN_MAX")) : kSmallChainAutoOutputs;
    int small_chain_tile = getenv("SDRHIP_SMALL_CHAIN_TILE") ? atoi(getenv("SDRHIP_SMALL_CHAIN_TILE")) : 0;
    // does a mode (0 / 1 / 2 = auto: up to auto_max audio outputs) want a run of n_out outputs?
    static bool mode_takes(int mode, int64_t n_out, int64_t auto_max) { return mode != 0 && (mode != 2 || n_out <= auto_max); }
    // set when the chain is created: resampler and audio filter have the shape both fused kernels are written for (AVX orders)
    bool fm_tail = false;
    // The tuner: `period` (re, im) pairs, 0 = none.  The device copy is made by the first run after set_tuner (a chain, tuned or
    // not, can be created and planned on a host without a GPU) and lives until the next set_tuner or the chain's end.
    int tuner_period = 0;
    std::vector<float> h_osc;
    float* d_osc = nullptr;
    bool tuner_pskip_ok = false;       // no mixed sample can overflow: the zero tap the constructor padded may be skipped (mac_window's PSKIP)
    int ensure_osc()
    {
        if (tuner_period == 0 || d_osc != nullptr) return SDRHIP_OK;
        return upload_floats(&d_osc, h_osc);
    }
    // the tuner's fused tile kernel (kernels_tuner.hip) serves this chain's decimator; whether it serves a LAUNCH also depends on
    // the alignment of that launch's first window (tuner_fused_fits)
    bool tuner_tile_shape() const { return decim.corder == CO_L4; }
    FmTailTables tail_tables() const      // their device tables (after ensure_device)
    {
        return {resamp.d_groups, resamp.row_stride, resamp.d_plain, resamp.ntaps, resamp.Lp, audio.d_taps, audio.d_cross, gain, block};
    }
    // Two runs in flight (sdrhip_fm_chain_set_overlap, round 4): consecutive runs alternate between two internal streams
    // ("lanes") and the two halves of the workspace, so the memory-heavy tail kernels of run k execute beside the power-bound
    // decimator of run k+1.  Consecutive runs of a stream are independent given their raw input (fm.hs:34-41: a block's
    // audio needs nothing of the previous block's results), which is what makes this legal.
    int overlap = 0;
    hipStream_t lane[2] = {nullptr, nullptr};
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    bool lane_busy[2] = {false, false};
    unsigned run_idx = 0;
    int ensure_lanes()
    {
        if (lane[0]) return SDRHIP_OK;
        for (int j = 0; j < 2; j++) {
            SDRHIP_CHECK_HIP(hipStreamCreateWithFlags(&lane[j], hipStreamNonBlocking));
            SDRHIP_CHECK_HIP(hipEventCreateWithFlags(&ev_in[j], hipEventDisableTiming));
            SDRHIP_CHECK_HIP(hipEventCreateWithFlags(&ev_out[j], hipEventDisableTiming));
        }
        return SDRHIP_OK;
    }

    // optional per-stage timing with HIP events on the stream each kernel is launched on
    bool timing = false;
    struct Span { Stage stage; hipEvent_t b, e; };
    std::vector<hipEvent_t> ev_pool;     // all timing events ever created
    size_t ev_used = 0;
    std::vector<Span> spans;             // recorded since the last read
    int runs = 0;
    int record_event(hipEvent_t* ev, hipStream_t s)
    {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e;
            SDRHIP_CHECK_HIP(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
        *ev = ev_pool[ev_used++];
        SDRHIP_CHECK_HIP(hipEventRecord(*ev, s));
        return SDRHIP_OK;
    }
    // launch() between the two events of a span of `stage` on stream s (timing off: launch() alone)
    template <class F>
    int timed(Stage stage, hipStream_t s, F&& launch)
    {
        Span sp{stage, nullptr, nullptr};
        int rc;
        if (timing && (rc = record_event(&sp.b, s)) != SDRHIP_OK) return rc;
        if ((rc = launch()) != SDRHIP_OK) return rc;
        if (!timing) return SDRHIP_OK;
        if ((rc = record_event(&sp.e, s)) != SDRHIP_OK) return rc;
        spans.push_back(sp);
        return SDRHIP_OK;
    }
    ~sdrhip_fm_chain()
    {
        for (int j = 0; j < 2; j++) {
            if (lane[j]) (void)hipStreamSynchronize(lane[j]);
            if (ev_in[j]) (void)hipEventDestroy(ev_in[j]);
            if (ev_out[j]) (void)hipEventDestroy(ev_out[j]);
            if (lane[j]) (void)hipStreamDestroy(lane[j]);
        }
        for (auto ev : ev_pool) (void)hipEventDestroy(ev);
        if (d_osc) (void)hipFree(d_osc);
    }

    // reach of resampler output m in y: the One kernel walks nloop floats, the Cross
    // kernel at most ceil(ntaps/I) <= nloop
    int y_reach() const { return resamp.nloop; }

    // first input sample in the receptive field of audio output q
    int64_t start(int64_t q) const
    {
        int64_t k = tail_first_y(resamp, q);
        if (k > 0) k -= 1;  // fmDemod looks one decimator output back (Demod.hs:28)
        return k * decim.factor;
    }
    // one past the last input sample in the receptive field of audio output q
    int64_t end(int64_t q) const
    {
        int64_t k_last = tail_end_y(resamp, audio, q) - 1;
        return k_last * decim.factor + decim.Lp;
    }
    // smallest q with start(q) >= s
    int64_t first_q_from(int64_t s) const
    {
        if (s <= 0) return 0;
        int64_t lo = 0, hi = (s / decim.factor + 2) * resamp.I / resamp.D + 4;
        while (start(hi) < s) hi *= 2;
        while (lo < hi) {
            int64_t mid = lo + (hi - lo) / 2;
            if (start(mid) >= s) hi = mid; else lo = mid + 1;
        }
        return lo;
    }
    // number of audio outputs that exist for a stream of total_in samples (by data
    // availability; the Pipes additionally withhold a trailing partial block)
    int64_t total_q(int64_t total_in) const
    {
        if (total_in < 0) return INT64_MAX / 4;
        if (total_in < decim.Lp) return 0;
        int64_t K = (total_in - decim.Lp) / decim.factor + 1;           // decimator outputs == demod outputs
        if (K * resamp.I < resamp.Lp) return 0;
        int64_t M = (K * resamp.I - resamp.Lp) / resamp.D + 1;          // resampler outputs
        if (M < audio.Lp) return 0;
        return M - audio.Lp + 1;
    }
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

extern "C" {

int sdrhip_fm_chain_create(sdrhip_fm_chain** c, int order, int decim_factor, const float* decim_taps, int n_decim_taps,
                           int interpolation, int decimation, const float* resamp_taps, int n_resamp_taps,
                           const float* audio_half_taps, int n_audio_half, float gain, int64_t block)
{
    SDRHIP_REQUIRE(c != nullptr, "sdrhip_fm_chain_create");
    *c = nullptr;
    SDRHIP_REQUIRE(block >= 0, "sdrhip_fm_chain_create");
    sdrhip_fm_chain* ch = new sdrhip_fm_chain();
    int rc = fir_create(&ch->decim, order, true, decim_factor, decim_taps, n_decim_taps);
    if (rc == SDRHIP_OK) rc = resamp_create(&ch->resamp, order, false, interpolation, decimation, resamp_taps, n_resamp_taps);
    if (rc == SDRHIP_OK) rc = fir_sym_create(&ch->audio, order, 1, audio_half_taps, n_audio_half);
    if (rc == SDRHIP_OK && block != 0 &&
        !(block >= ch->decim.Lp && block * ch->resamp.I >= ch->resamp.Lp && block >= ch->audio.Lp)) {
        set_error("sdrhip_fm_chain_create: block %lld shorter than a stage's filter (Filter.hs:544,586,691)", (long long)block);
        rc = SDRHIP_ERR_ARG;
    }
    if (rc != SDRHIP_OK) { delete ch; return rc; }
    ch->gain = gain;
    ch->block = block;
    const ResampDesc& r = ch->resamp;
    const FirDesc& a = ch->audio;
    ch->fm_tail = !r.cplx && r.lanes == 8 && !a.cplx && a.sym && a.lanes == 8 && a.factor == 1 &&
                  fm_tail_shape_ok(r.num_groups, r.nloop, r.I, r.D, r.increments.data(), r.Lp, r.ntaps, a.ntaps_kernel);
    *c = ch;
    return SDRHIP_OK;
}

void sdrhip_fm_chain_destroy(sdrhip_fm_chain* c) { delete c; }

int sdrhip_fm_chain_plan(const sdrhip_fm_chain* c, int64_t s0, int64_t s1, int64_t total_in, int64_t* q0, int64_t* q1,
                         int64_t* halo)
{
    SDRHIP_REQUIRE(c != nullptr && q0 && q1 && halo, "sdrhip_fm_chain_plan");
    SDRHIP_REQUIRE(s0 >= 0 && s1 >= s0, "sdrhip_fm_chain_plan");
    int64_t Q = c->total_q(total_in);
    int64_t a = c->first_q_from(s0), b = c->first_q_from(s1);
    if (a > Q) a = Q;
    if (b > Q) b = Q;
    *q0 = a;
    *q1 = b;
    int64_t h = 0;
    if (b > a) {
        h = c->end(b - 1) - s1;
        if (h < 0) h = 0;
    }
    *halo = h;
    return SDRHIP_OK;
}

int64_t sdrhip_fm_chain_ready(const sdrhip_fm_chain* c, int64_t n_samples)
{
    if (!c || n_samples < 0) return -1;
    return ready_by_end([c](int64_t q) { return c->end(q); }, n_samples);      // end() is non-decreasing
}

int64_t sdrhip_fm_chain_max_halo(const sdrhip_fm_chain* c)
{
    if (!c) return -1;
    return longest_field([c](int64_t q) { return c->start(q); }, [c](int64_t q) { return c->end(q); }, c->resamp.I);
}

int64_t sdrhip_fm_chain_halo_samples(const sdrhip_fm_chain* c)
{
    const int64_t h = sdrhip_fm_chain_max_halo(c);
    return h < 0 ? h : (h + 7) / 8 * 8;      // whole 16-byte vectors of u8 IQ, the same on every rank
}

int sdrhip_fm_chain_halo_exchange(const sdrhip_fm_chain* chain, sdrhip_comm* comm, void* stream, uint8_t* d_buf, int64_t shard_samples)
{
    SDRHIP_REQUIRE(chain != nullptr && comm != nullptr && d_buf != nullptr && shard_samples > 0, "sdrhip_fm_chain_halo_exchange");
    const int64_t halo = sdrhip_fm_chain_halo_samples(chain);
    SDRHIP_REQUIRE(halo <= shard_samples, "sdrhip_fm_chain_halo_exchange: shard shorter than the halo");
    return sdrhip_halo_exchange(comm, stream, d_buf, d_buf + 2 * shard_samples, (size_t)(2 * halo));
}

size_t sdrhip_fm_chain_halo_staging_bytes(const sdrhip_fm_chain* chain, int count)
{
    if (!chain || count < 1) return 0;
    return 2 * (size_t)count * (size_t)(2 * sdrhip_fm_chain_halo_samples(chain));
}

int sdrhip_fm_chain_halo_exchange_batch(const sdrhip_fm_chain* chain, sdrhip_comm* comm, void* stream, uint8_t* d_buf, int64_t shard_samples,
                                        size_t row_bytes, int count, void* d_staging)
{
    SDRHIP_REQUIRE(chain != nullptr && comm != nullptr && d_buf != nullptr && shard_samples > 0 && count >= 1, "sdrhip_fm_chain_halo_exchange_batch");
    const size_t hb = (size_t)(2 * sdrhip_fm_chain_halo_samples(chain));            // bytes of one halo
    SDRHIP_REQUIRE((int64_t)hb <= 2 * shard_samples, "sdrhip_fm_chain_halo_exchange_batch: shard shorter than the halo");
    if (count == 1) return sdrhip_halo_exchange(comm, stream, d_buf, d_buf + 2 * shard_samples, hb);
    SDRHIP_REQUIRE(d_staging != nullptr && row_bytes >= (size_t)(2 * shard_samples) + hb, "sdrhip_fm_chain_halo_exchange_batch: rows hold a shard and its halo");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* send = (uint8_t*)d_staging;
    uint8_t* recv = send + (size_t)count * hb;
    // heads of the count rows -> one contiguous message; the received message -> the count halo regions
    SDRHIP_CHECK_HIP(hipMemcpy2DAsync(send, hb, d_buf, row_bytes, hb, (size_t)count, hipMemcpyDeviceToDevice, s));
    const int rc = sdrhip_halo_exchange(comm, stream, send, recv, (size_t)count * hb);
    if (rc != SDRHIP_OK) return rc;
    SDRHIP_CHECK_HIP(hipMemcpy2DAsync(d_buf + 2 * shard_samples, row_bytes, recv, hb, hb, (size_t)count, hipMemcpyDeviceToDevice, s));
    return SDRHIP_OK;
}

size_t sdrhip_fm_chain_workspace_bytes(const sdrhip_fm_chain* c, int64_t n_in)
{
    if (!c || n_in < 0) return 0;
    int64_t nk = n_in / c->decim.factor + 4;
    int64_t nm = nk * c->resamp.I / c->resamp.D + 4;
    // unfused first stage: the converted input (+ 16 filter lengths with their alignment padding: what round 4's sub-batches recomputed;
    // no run needs it any more, but the size callers allocate stays what it was)
    // a tuned chain reserves the same region for the mixed samples whatever its first stage: a launch whose first window is not
    // 16-byte aligned cannot take the tuner's tile kernel, and the size is asked for before any launch is known
    const size_t conv = c->fused_first_stage() && c->tuner_period == 0 ? 0 : align_up((size_t)(n_in + 16) * 8, 256) + 16 * align_up((size_t)(c->decim.Lp + 16) * 8, 256);
    const size_t one = conv + align_up((size_t)nk * 8, 256) + align_up((size_t)nk * 4, 256) + align_up((size_t)nm * 4, 256) + 256 + 16 * (64 << 10);
    return c->overlap ? 2 * align_up(one, 256) : one;      // two runs in flight: one half per lane
}

namespace {
// The stage ranges of one run, back to front from the audio outputs [q0, q1), and where the stage routes keep them
struct RunPlan {
    int64_t m1;                          // resampler outputs z[q0, m1)
    int64_t ky0, ky1;                    // demod outputs
    int64_t kd0, kd1;                    // decimator outputs (fmDemod looks one back)
    int64_t n_lo, n_hi;                  // the input samples the run reads
    int64_t xa = 0, xb = 0;              // staged first stage only: samples [xa, xb) of the stream are converted (tuned: mixed) to the workspace's start
    bool tuner_tile = false;             // tuned chain: the first stage is the tuner's fused tile kernel
    size_t off_d = 0, off_y, off_z;      // decimated, demodulated, resampled
    size_t ws_need;                      // bytes of workspace the stage routes use
};
}  // namespace

// The first stage of a tuned run as the tuner sees it: decimator outputs [kd0, kd1) from u8 IQ whose sample 0 is stream index s0
static Geom tuner_geom(const sdrhip_fm_chain* c, int64_t s0, int64_t kd0, int64_t kd1)
{
    Geom g;
    g.in_base = s0;
    g.k_begin = kd0;
    g.count = (int)(kd1 - kd0);
    g.I = 1;
    g.D = c->decim.factor;
    g.Lp = c->decim.Lp;
    g.seamBI = c->block;
    return g;
}

// d_in_iq, d_workspace: only their alignment counts (a tuned run takes the tuner's tile kernel where its 16-byte loads are aligned).
// fmt: IN_U8, or IN_I16 for the runs of a receiver bank on 16-bit signed IQ (tuned chains only; the int16 tile kernel's predicate)
static RunPlan plan_run(const sdrhip_fm_chain* c, int64_t s0, int64_t q0, int64_t q1, const void* d_in_iq, const void* d_workspace,
                        InFmt fmt = IN_U8)
{
    RunPlan r;
    r.m1 = q1 + c->audio.Lp - 1;
    r.ky0 = c->resamp.in_offset(q0);
    r.ky1 = c->resamp.in_offset(r.m1 - 1) + c->y_reach();
    r.kd0 = r.ky0 > 0 ? r.ky0 - 1 : 0;
    r.kd1 = r.ky1;
    r.n_lo = r.kd0 * c->decim.factor;
    r.n_hi = (r.kd1 - 1) * c->decim.factor + c->decim.Lp;
    bool staged = !c->fused_first_stage();      // the first stage reads cfloat samples from the workspace's start
    if (c->tuner_period != 0) {
        const Geom g = tuner_geom(c, s0, r.kd0, r.kd1);
        r.tuner_tile = c->tuner_tile_shape() && r.kd1 - r.kd0 < (int64_t)0x7fffffff &&
                       tuner_fused_fits(g, c->decim.Lp, true, d_in_iq, fmt, d_workspace, c->tuner_period);
        staged = !r.tuner_tile;
    }
    if (staged) {
        r.xa = s0 + ((r.n_lo - s0) & ~(int64_t)7);                   // 16-byte aligned in the u8 stream
        r.xb = r.n_hi;
        r.off_d = align_up((size_t)(r.xb - r.xa) * 8, 256);
    }
    r.off_y = r.off_d + align_up((size_t)(r.kd1 - r.kd0) * 8, 256);
    r.off_z = r.off_y + align_up((size_t)(r.ky1 - r.ky0) * 4, 256);
    r.ws_need = r.off_z + align_up((size_t)(r.m1 - q0) * 4, 256);
    return r;
}

// the end of every route: the first failure, or what the launches left in HIP's error state
static int launched(int rc)
{
    if (rc != SDRHIP_OK) return rc;
    SDRHIP_CHECK_HIP(hipGetLastError());
    return SDRHIP_OK;
}

// does the one-kernel chain (kernels_small.hip) serve a run of this chain on this input?  (the tuned one reads the plain taps: it
// needs no exactly pre-scaled ones)
static bool chain_small_fits(const sdrhip_fm_chain* c, const uint8_t* d_in_iq, int64_t s0)
{
    const FirDesc& dec = c->decim;
    return c->fm_tail && fm_chain_small_fits(dec.factor, dec.Lp, dec.corder, c->tuner_period != 0 || !dec.h_scaled.empty(), c->block, d_in_iq, s0);
}

// does d_in hold the receptive field of the run's outputs?  (it depends on no table: the receiver bank asks once for all stations)
static int input_holds(const char* who, const RunPlan& r, int64_t s0, int64_t n_in, int64_t q0, int64_t q1)
{
    if (r.n_lo >= s0 && r.n_hi <= s0 + n_in) return SDRHIP_OK;
    set_error("%s: outputs [%lld,%lld) need samples [%lld,%lld) but d_in holds [%lld,%lld)", who, (long long)q0, (long long)q1,
              (long long)r.n_lo, (long long)r.n_hi, (long long)s0, (long long)(s0 + n_in));
    return SDRHIP_ERR_ARG;
}

// The route of one run of at least one output, and EVERY refusal of such a run: chain_run_on launches only after this, and the
// receiver bank asks it for all its stations before the first one runs, so that a refused bank run has written no row.  A new
// refusal belongs here.  who: the public call the message names.
struct RunRoute {
    RunPlan r;
    bool small = false, tail = false;     // the first of the two fused kernels that is wanted (mode and size) and fits, else the stage kernels
};
static int chain_route(const sdrhip_fm_chain* c, const char* who, const uint8_t* d_in_iq, int64_t s0, int64_t n_in, const float* d_audio,
                       int64_t q0, int64_t q1, const void* d_workspace, size_t workspace_bytes, RunRoute* out, InFmt fmt = IN_U8)
{
    SDRHIP_REQUIRE(d_in_iq && d_audio && d_workspace, who);
    SDRHIP_REQUIRE(fmt == IN_U8 || (fmt == IN_I16 && c->tuner_period != 0), who);      // int16 reaches a chain through its bank only
    RunRoute& t = *out;
    t.r = plan_run(c, s0, q0, q1, d_in_iq, d_workspace, fmt);
    int rc;
    if ((rc = input_holds(who, t.r, s0, n_in, q0, q1)) != SDRHIP_OK) return rc;
    // int16: the one-kernel chain exists in the bank's form only (the banked launch, bank_run); a station's own run starts with the
    // tuner's int16 first stage and goes on as any run
    t.small = fmt == IN_U8 && c->mode_takes(c->small_chain, q1 - q0, c->small_chain_max) && chain_small_fits(c, d_in_iq, s0);
    t.tail = !t.small && c->fm_tail && c->mode_takes(c->fused_tail, q1 - q0, kFusedTailAutoOutputs) && fm_tail_fused_fits(c->resamp.Lp, c->block);
    if (!t.small && t.r.ws_need > workspace_bytes) {       // the one-kernel chain sends nothing through the workspace
        set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, t.r.ws_need);
        return SDRHIP_ERR_ARG;
    }
    if (c->tuner_period != 0 && !t.small && !t.r.tuner_tile && t.r.xb - t.r.xa >= (int64_t)0x7fffffff) {
        set_error("%s: a tuned run that mixes into the workspace takes fewer than 2^31 samples", who);
        return SDRHIP_ERR_ARG;
    }
    return SDRHIP_OK;
}

// input_over_link: d_in_iq is pinned HOST memory (the host-block operator's in-place pushes): the one-kernel chain takes its largest tile.
// fmt == IN_I16 (a receiver bank's station-by-station route on 16-bit signed IQ): d_in_iq holds interleaved int16, 4 bytes per sample;
// the first stage is the tuner's on such input, everything behind it is the same code.
static int chain_run_on(sdrhip_fm_chain* c, void* stream, const uint8_t* d_in_iq, int64_t s0, int64_t n_in, float* d_audio,
                        int64_t q0, int64_t q1, void* d_workspace, size_t workspace_bytes, bool input_over_link, InFmt fmt = IN_U8)
{
    SDRHIP_REQUIRE(q1 >= q0 && q0 >= 0 && s0 >= 0 && n_in >= 0, "sdrhip_fm_chain_run");
    if (q1 == q0) return SDRHIP_OK;
    hipStream_t s = (hipStream_t)stream;

    RunRoute route;
    int rc;
    if ((rc = chain_route(c, "sdrhip_fm_chain_run", d_in_iq, s0, n_in, d_audio, q0, q1, d_workspace, workspace_bytes, &route, fmt)) != SDRHIP_OK) return rc;
    const RunPlan& r = route.r;
    const bool small = route.small, tail = route.tail;
    const FirDesc& dec = c->decim;
    const bool tuned = c->tuner_period != 0;
    if (small || tail)
        if ((rc = c->resamp.ensure_device()) != SDRHIP_OK || (rc = c->audio.ensure_device()) != SDRHIP_OK) return rc;
    if (tuned)
        if ((rc = dec.ensure_device()) != SDRHIP_OK || (rc = c->ensure_osc()) != SDRHIP_OK) return rc;
    if (c->timing) c->runs++;

    if (small) {      // launch-bound run: the whole chain in ONE kernel
        if ((rc = dec.ensure_device()) != SDRHIP_OK) return rc;
        return launched(c->timed(kFusedChain, s, [&] {
            const int tile = c->small_chain_tile != 0 ? c->small_chain_tile : (input_over_link ? -1 : 0);
            if (tuned)
                launch_fm_chain_small(s, d_in_iq, s0, n_in, d_audio, q0, q1, dec.d_plain, dec.last_tap_is_padding() && c->tuner_pskip_ok,
                                      c->tail_tables(), tile, c->d_osc, c->tuner_period);
            else
                launch_fm_chain_small(s, d_in_iq, s0, n_in, d_audio, q0, q1, dec.d_scaled, dec.last_tap_is_padding(), c->tail_tables(), tile);
            return SDRHIP_OK;
        }));
    }

    char* ws = (char*)d_workspace;
    float* d_d = (float*)(ws + r.off_d);
    float* d_y = (float*)(ws + r.off_y);
    float* d_z = (float*)(ws + r.off_z);
    // K1+K2: u8 -> cfloat -> decimate (convert.c:37-50 fused into decimate.c:105-113)
    rc = c->timed(kDecimate, s, [&] {
        if (tuned) {
            // the tuner's own routes on the caller's workspace and this run's stream (no leased scratch, no events: runs are captured
            // into graphs and alternate between the overlap lanes): its tile kernel (for int16 the bank's with one channel), or the mix
            // into the workspace's start and the stock cfloat decimator on it
            if (r.tuner_tile) {
                if (!launch_tuner_fused(s, tuner_geom(c, s0, r.kd0, r.kd1), dec.d_plain, dec.Lp, dec.d_cross, d_in_iq, fmt, d_d, c->d_osc, c->tuner_period)) {
                    set_error(fmt == IN_I16 ? "sdrhip_fm_bank_run_i16: the tuner's int16 tile kernel refused a launch its predicate accepted"
                                            : "sdrhip_fm_chain_run: the tuner's tile kernel refused a launch its predicate accepted");
                    return SDRHIP_ERR_STATE;
                }
                return SDRHIP_OK;
            }
            launch_tuner_mix(s, d_in_iq + in_fmt_bytes(fmt) * (r.xa - s0), fmt, (float*)ws, r.xb - r.xa, c->d_osc, c->tuner_period,
                             (int)(r.xa % c->tuner_period));
            return fir_run(&dec, s, ws, false, r.xa, d_d, r.kd0, r.kd1, c->block);
        }
        if (c->fused_first_stage()) return fir_run(&dec, s, d_in_iq, true, s0, d_d, r.kd0, r.kd1, c->block);
        launch_convert_u8(s, d_in_iq + 2 * (r.xa - s0), (float*)ws, 2 * (r.xb - r.xa));
        return fir_run(&dec, s, ws, false, r.xa, d_d, r.kd0, r.kd1, c->block);
    });
    if (rc != SDRHIP_OK) return rc;
    const float* d_iq = d_d + 2 * (r.ky0 - r.kd0);      // the decimator output whose phase step is y[ky0]
    if (tail)
        return launched(c->timed(kFusedTail, s, [&] {
            launch_fm_tail_fused(s, d_d, r.kd0, r.kd1, r.ky0, r.ky1, d_audio, q0, q1, c->tail_tables());
            return SDRHIP_OK;
        }));
    if (c->fuse_demod) {
        // K3+K4: fmDemod inside the resampler's tile loader on large batches (y never reaches HBM), a stand-alone fmDemod launch first otherwise
        rc = c->timed(kResample, s, [&] {
            return resamp_run_demod(&c->resamp, s, d_iq, r.ky0 > r.kd0, r.ky1 - r.ky0, d_y, r.ky0, d_z, q0, r.m1, c->block, c->block, nullptr);
        });
    } else {
        // K3: fmDemod; at stream start the carried sample is 0 (Demod.hs:41)
        rc = c->timed(kFmDemod, s, [&] {
            launch_fm_demod_fast(s, d_iq, d_y, r.ky1 - r.ky0, r.ky0 > r.kd0, 0.0f, 0.0f);
            return SDRHIP_OK;
        });
        // K4: polyphase resample
        if (rc == SDRHIP_OK) rc = c->timed(kResample, s, [&] { return resamp_run(&c->resamp, s, d_y, r.ky0, d_z, q0, r.m1, c->block, c->block); });
    }
    // K5: symmetric audio filter (+ fm.hs:40 `P.map (VG.map (* 0.2))` as the kernel's epilogue: a separate f32 multiply of the rounded output)
    if (rc == SDRHIP_OK) rc = c->timed(kFilter, s, [&] { return fir_run(&c->audio, s, d_z, false, q0, d_audio, q0, q1, c->block, c->gain); });
    return launched(rc);
}

// One run in the chain's current mode; sdrhip_fm_chain_run and the host-block operator's submissions
static int chain_run(sdrhip_fm_chain* c, void* stream, const uint8_t* d_in_iq, int64_t s0, int64_t n_in, float* d_audio, int64_t q0,
                     int64_t q1, void* d_workspace, size_t workspace_bytes, bool input_over_link, InFmt fmt = IN_U8)
{
    if (!c->overlap) return chain_run_on(c, stream, d_in_iq, s0, n_in, d_audio, q0, q1, d_workspace, workspace_bytes, input_over_link, fmt);
    // two runs in flight: this run goes to lane j, after everything queued on the caller's stream so far (its input's
    // producer); the caller's stream is then made to wait for the PREVIOUS run (lane 1 - j), not for this one
    hipStream_t s = (hipStream_t)stream;
    int rc = c->ensure_lanes();
    if (rc != SDRHIP_OK) return rc;
    const int j = (int)(c->run_idx++ & 1u);
    SDRHIP_CHECK_HIP(hipEventRecord(c->ev_in[j], s));
    SDRHIP_CHECK_HIP(hipStreamWaitEvent(c->lane[j], c->ev_in[j], 0));
    const size_t half = (workspace_bytes / 2) & ~(size_t)255;
    rc = chain_run_on(c, (void*)c->lane[j], d_in_iq, s0, n_in, d_audio, q0, q1, d_workspace ? (char*)d_workspace + (size_t)j * half : nullptr, half,
                      input_over_link, fmt);
    // (also when the run failed half way: kernels it did enqueue on the lane may still be reading the input and writing the
    // audio and the workspace half, and a later run or join must be ordered behind them)
    const hipError_t erec = hipEventRecord(c->ev_out[j], c->lane[j]);
    c->lane_busy[j] = true;
    if (rc != SDRHIP_OK) return rc;
    SDRHIP_CHECK_HIP(erec);
    if (c->lane_busy[1 - j]) SDRHIP_CHECK_HIP(hipStreamWaitEvent(s, c->ev_out[1 - j], 0));
    return SDRHIP_OK;
}

int sdrhip_fm_chain_run(sdrhip_fm_chain* c, void* stream, const uint8_t* d_in_iq, int64_t s0, int64_t n_in,
                        float* d_audio, int64_t q0, int64_t q1, void* d_workspace, size_t workspace_bytes)
{
    SDRHIP_REQUIRE(c != nullptr, "sdrhip_fm_chain_run");
    return chain_run(c, stream, d_in_iq, s0, n_in, d_audio, q0, q1, d_workspace, workspace_bytes, false);
}

int sdrhip_fm_chain_join(sdrhip_fm_chain* c, void* stream)
{
    SDRHIP_REQUIRE(c != nullptr, "sdrhip_fm_chain_join");
    for (int j = 0; j < 2; j++)
        if (c->lane_busy[j]) {
            SDRHIP_CHECK_HIP(hipStreamWaitEvent((hipStream_t)stream, c->ev_out[j], 0));
            c->lane_busy[j] = false;
        }
    return SDRHIP_OK;
}

int sdrhip_fm_chain_set_overlap(sdrhip_fm_chain* c, int on)
{
    SDRHIP_REQUIRE(c != nullptr && (on == 0 || on == 1), "sdrhip_fm_chain_set_overlap");
    // switching modes with runs still in flight: drain them first (a host-side wait; this is a configuration call)
    for (int j = 0; j < 2; j++)
        if (c->lane_busy[j]) {
            SDRHIP_CHECK_HIP(hipStreamSynchronize(c->lane[j]));
            c->lane_busy[j] = false;
        }
    c->overlap = on;
    return SDRHIP_OK;
}

// ---- one run with fixed arguments as a hipGraph: launch-bound batches (a 2^20-sample shard is nine small kernels) pay one
// graph launch instead of nine kernel launches.  Captured from the very code path sdrhip_fm_chain_run takes.
struct sdrhip_fm_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t cap = nullptr;
    ~sdrhip_fm_graph()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        if (cap) (void)hipStreamDestroy(cap);
    }
};

int sdrhip_fm_chain_graph_create(sdrhip_fm_graph** out, sdrhip_fm_chain* c, const uint8_t* d_in_iq, int64_t s0, int64_t n_in, float* d_audio,
                                 int64_t q0, int64_t q1, void* d_workspace, size_t workspace_bytes)
{
    SDRHIP_REQUIRE(out != nullptr && c != nullptr, "sdrhip_fm_chain_graph_create");
    *out = nullptr;
    SDRHIP_REQUIRE(!c->timing && !c->overlap, "sdrhip_fm_chain_graph_create: per-stage timing and two runs "
                                               "in flight record events on the chain's own streams: switch them off for a captured run");
    sdrhip_fm_graph* g = new sdrhip_fm_graph();
    hipError_t e = hipStreamCreateWithFlags(&g->cap, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error("sdrhip_fm_chain_graph_create: %s", hipGetErrorString(e)); delete g; return SDRHIP_ERR_HIP; }
    // a plain run first: tap uploads, kernel attributes and argument checks happen outside the capture
    int rc = sdrhip_fm_chain_run(c, (void*)g->cap, d_in_iq, s0, n_in, d_audio, q0, q1, d_workspace, workspace_bytes);
    if (rc == SDRHIP_OK && hipStreamSynchronize(g->cap) != hipSuccess) { set_error("sdrhip_fm_chain_graph_create: warm-up run failed"); rc = SDRHIP_ERR_HIP; }
    if (rc != SDRHIP_OK) { delete g; return rc; }
    e = hipStreamBeginCapture(g->cap, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { set_error("hipStreamBeginCapture: %s", hipGetErrorString(e)); delete g; return SDRHIP_ERR_HIP; }
    rc = sdrhip_fm_chain_run(c, (void*)g->cap, d_in_iq, s0, n_in, d_audio, q0, q1, d_workspace, workspace_bytes);
    e = hipStreamEndCapture(g->cap, &g->graph);
    if (rc != SDRHIP_OK) { delete g; return rc; }
    if (e != hipSuccess || g->graph == nullptr) { set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); delete g; return SDRHIP_ERR_HIP; }
    e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); delete g; return SDRHIP_ERR_HIP; }
    *out = g;
    return SDRHIP_OK;
}

int sdrhip_fm_chain_graph_launch(sdrhip_fm_graph* g, void* stream)
{
    SDRHIP_REQUIRE(g != nullptr && g->exec != nullptr, "sdrhip_fm_chain_graph_launch");
    SDRHIP_CHECK_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
    return SDRHIP_OK;
}

void sdrhip_fm_chain_graph_destroy(sdrhip_fm_graph* g) { delete g; }

int sdrhip_fm_chain_set_fused_tail(sdrhip_fm_chain* c, int enable)
{
    SDRHIP_REQUIRE(c != nullptr && enable >= 0 && enable <= 2, "sdrhip_fm_chain_set_fused_tail");
    c->fused_tail = enable;
    return SDRHIP_OK;
}

int sdrhip_fm_chain_set_small_chain(sdrhip_fm_chain* c, int mode, int64_t max_outputs, int tile_outputs)
{
    SDRHIP_REQUIRE(c != nullptr && mode >= 0 && mode <= 2 && tile_outputs >= 0, "sdrhip_fm_chain_set_small_chain");
    c->small_chain = mode;
    c->small_chain_max = max_outputs > 0 ? max_outputs : kSmallChainAutoOutputs;
    c->small_chain_tile = tile_outputs;
    return SDRHIP_OK;
}

long long sdrhip_debug_small_chain_launches(void) { return fm_chain_small_launch_count(); }
long long sdrhip_debug_small_chain_tuned_launches(void) { return fm_chain_small_tuned_launch_count(); }
long long sdrhip_debug_fused_tail_launches(void) { return fm_tail_launch_count(); }
long long sdrhip_debug_resample_cycle_launches(void) { return resample_cycle_launch_count(); }
long long sdrhip_debug_decimate_real16_launches(void) { return decimate_real16_launch_count(); }
void sdrhip_debug_set_systolic(int on) { set_systolic(on); }
long long sdrhip_debug_systolic_launches(void) { return systolic_launch_count(); }
long long sdrhip_debug_systolic_plain_launches(void) { return systolic_plain_launch_count(); }
long long sdrhip_debug_decimator_crossfix_launches(void) { return decimator_crossfix_launch_count(); }
long long sdrhip_debug_fused_demod_launches(void) { return fused_demod_launch_count(); }
long long sdrhip_debug_generic_u8_launches(void) { return generic_u8_launch_count(); }
void sdrhip_debug_systolic_plan(int count, int* nstrips, int* nwhole) { systolic_plan(count, nstrips, nwhole); }

int sdrhip_fm_chain_set_tuner(sdrhip_fm_chain* c, const float* osc_iq, int period)
{
    SDRHIP_REQUIRE(c != nullptr, "sdrhip_fm_chain_set_tuner");
    SDRHIP_REQUIRE(period >= 0 && period <= 65536, "sdrhip_fm_chain_set_tuner: period 1 .. 65536 (0 with a null table: no tuner)");
    SDRHIP_REQUIRE((osc_iq == nullptr) == (period == 0), "sdrhip_fm_chain_set_tuner: a table and its period, or (NULL, 0)");
    // |x| <= 1 for converted u8, so a mixed component is at most |re| + |im| in magnitude: while that is finite no sample overflows
    bool no_overflow = true;
    for (size_t i = 0; i < 2 * (size_t)period; i++) {
        SDRHIP_REQUIRE(isfinite(osc_iq[i]), "sdrhip_fm_chain_set_tuner: non-finite table entry");
        if (i % 2 == 1 && fabs((double)osc_iq[i - 1]) + fabs((double)osc_iq[i]) > (double)FLT_MAX) no_overflow = false;
    }
    // no run of this chain is in flight (the caller's side of the contract): the old table can go.  hipFree waits for the device.
    if (c->d_osc) {
        SDRHIP_CHECK_HIP(hipFree(c->d_osc));
        c->d_osc = nullptr;
    }
    c->h_osc.assign(osc_iq, osc_iq + 2 * (size_t)period);
    c->tuner_period = period;
    c->tuner_pskip_ok = no_overflow;
    return SDRHIP_OK;
}

int sdrhip_fm_chain_tuner_period(const sdrhip_fm_chain* c) { return c ? c->tuner_period : SDRHIP_ERR_ARG; }

int sdrhip_fm_chain_set_demod_fusion(sdrhip_fm_chain* c, int enable)
{
    SDRHIP_REQUIRE(c != nullptr, "sdrhip_fm_chain_set_demod_fusion");
    c->fuse_demod = enable != 0;
    return SDRHIP_OK;
}

int sdrhip_fm_chain_enable_timing(sdrhip_fm_chain* c, int enable)
{
    SDRHIP_REQUIRE(c != nullptr, "sdrhip_fm_chain_enable_timing");
    c->timing = enable != 0;
    c->spans.clear();
    c->ev_used = 0;
    c->runs = 0;
    return SDRHIP_OK;
}

int sdrhip_fm_chain_read_timing(sdrhip_fm_chain* c, double* ms_sum, int* runs)
{
    SDRHIP_REQUIRE(c != nullptr && ms_sum != nullptr && runs != nullptr, "sdrhip_fm_chain_read_timing");
    for (int i = 0; i < kStages; i++) ms_sum[i] = 0.0;
    for (const auto& sp : c->spans) {
        SDRHIP_CHECK_HIP(hipEventSynchronize(sp.e));
        float ms = 0.0f;
        SDRHIP_CHECK_HIP(hipEventElapsedTime(&ms, sp.b, sp.e));
        ms_sum[sp.stage] += ms;
    }
    *runs = c->runs;
    c->spans.clear();
    c->ev_used = 0;
    c->runs = 0;
    return SDRHIP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The receiver bank: every station of ONE capture.  K tuned chains of the same arguments, one oscillator table each, over one
// input.  Station j's audio row is, bit for bit, what a chain created with these arguments and sdrhip_fm_chain_set_tuner(table j)
// writes: the bank OWNS those K chains -- they answer plan / ready / max_halo / workspace_bytes and ARE the station-by-station
// route -- and one device copy of all the tables for the banked route, ONE launch of the one-kernel chain with a station axis in
// its grid (kernels_small.hip): K launch-bound runs for the launch latency of one.
//   banked route      where the tuned one-kernel chain fits (fm_chain_small_fits with tuned taps, the tail's shape, a grid that
//                     exists); auto takes it while outputs <= kBankAutoStationOutputs and stations * outputs <= max_outputs
//   station by station  sdrhip_fm_chain_run per station on the caller's stream and the caller's ONE workspace (the runs are ordered
//                     on the stream); every size and alignment the banked launch refuses, and large runs, which are bound by
//                     arithmetic and take the tuner's tile kernel as a tuned chain does
// ---------------------------------------------------------------------------
static_assert(SDRHIP_FM_BANK_MAX_STATIONS == kFmBankMaxStations, "the header's limit is the kernel's");
// auto is a rule in TWO dimensions: the banked launch while a station's run, q1 - q0, is at most kBankAutoStationOutputs AND
// stations * (q1 - q0) is at most max_outputs (built-in: kBankAutoOutputs).  Both are the edges of what was measured
// (tools/fm_bank_bench.py, profiles/fm_bank_bench.txt: 1 .. 32 stations x runs of 1 block, 16 blocks and 2^20 samples = 39322 outputs),
// not crossovers: inside that rectangle the banked launch is ahead of K runs of K tuned chains at every point with K > 1, its
// far corner included (32 x 39322 outputs, 201 against 443 us), and level at K = 1.  A longer run per station goes station by
// station whatever K is: nothing there is measured, a station is bound by arithmetic there, and beyond the chain's own
// kSmallChainAutoOutputs its chain leaves the one-kernel route for the stage kernels, which the banked launch cannot follow.
// (The chain's 159 * 1728 as the total, where this started, would have sent 8 stations x 2^20 samples station by station at 1.9
// times the time.)
static const int64_t kBankAutoStationOutputs = 39322;
static const int64_t kBankAutoOutputs = 32 * kBankAutoStationOutputs;
static_assert(kBankAutoStationOutputs <= kSmallChainAutoOutputs, "auto banks no run that the station's own chain would give to the stage kernels");

struct sdrhip_fm_bank {
    std::vector<sdrhip_fm_chain*> ch;       // station j as a tuned chain
    std::vector<float> h_tables;            // every table, back to back
    int off[SDRHIP_FM_BANK_MAX_STATIONS] = {0};      // station j's first (re, im) pair in h_tables / d_tables
    int period[SDRHIP_FM_BANK_MAX_STATIONS] = {0};
    float* d_tables = nullptr;              // made by the first banked run
    int route = 0;                          // 0 = auto, 1 = banked, 2 = station by station
    int64_t max_outputs = kBankAutoOutputs;
    int tile = 0;
    // the zero tap the constructor padded may be skipped only when no station's mixed samples can overflow
    bool pskip_ok() const
    {
        for (const sdrhip_fm_chain* c : ch)
            if (!c->tuner_pskip_ok) return false;
        return true;
    }
    // ... on 16-bit signed IQ: the chains' flag is decided under |x| <= 1, which holds for converted u8; converted int16 reaches
    // |x| = 16, so an int16 run may skip only while 16 (|re| + |im|) is finite in float for every entry of every table (set at create)
    bool pskip_ok_i16 = false;
    ~sdrhip_fm_bank()
    {
        for (sdrhip_fm_chain* c : ch) delete c;
        if (d_tables) (void)hipFree(d_tables);
    }
};

extern "C" {

int sdrhip_fm_bank_create(sdrhip_fm_bank** b, int order, int decim_factor, const float* decim_taps, int n_decim_taps, int interpolation,
                          int decimation, const float* resamp_taps, int n_resamp_taps, const float* audio_half_taps, int n_audio_half,
                          float gain, int64_t block, int stations, const float* const* osc_iq, const int* periods)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_fm_bank_create");
    *b = nullptr;
    SDRHIP_REQUIRE(stations >= 1 && stations <= SDRHIP_FM_BANK_MAX_STATIONS, "sdrhip_fm_bank_create: 1 .. 32 stations");
    SDRHIP_REQUIRE(osc_iq != nullptr && periods != nullptr, "sdrhip_fm_bank_create");
    for (int j = 0; j < stations; j++) {
        SDRHIP_REQUIRE(osc_iq[j] != nullptr, "sdrhip_fm_bank_create: every station has a table (a station on the centre: {1, 0})");
        SDRHIP_REQUIRE(periods[j] >= 1 && periods[j] <= 65536, "sdrhip_fm_bank_create: period 1 .. 65536");
        for (size_t i = 0; i < 2 * (size_t)periods[j]; i++)
            SDRHIP_REQUIRE(isfinite(osc_iq[j][i]), "sdrhip_fm_bank_create: non-finite table entry");
    }
    sdrhip_fm_bank* bk = new sdrhip_fm_bank();
    size_t pairs = 0;
    for (int j = 0; j < stations; j++) {
        sdrhip_fm_chain* c = nullptr;
        int rc = sdrhip_fm_chain_create(&c, order, decim_factor, decim_taps, n_decim_taps, interpolation, decimation, resamp_taps, n_resamp_taps,
                                        audio_half_taps, n_audio_half, gain, block);
        if (rc == SDRHIP_OK) {
            bk->ch.push_back(c);
            rc = sdrhip_fm_chain_set_tuner(c, osc_iq[j], periods[j]);
        }
        if (rc != SDRHIP_OK) { delete bk; return rc; }
        bk->off[j] = (int)pairs;
        bk->period[j] = periods[j];
        bk->h_tables.insert(bk->h_tables.end(), osc_iq[j], osc_iq[j] + 2 * (size_t)periods[j]);
        pairs += (size_t)periods[j];
    }
    bk->pskip_ok_i16 = true;
    for (size_t i = 0; i + 1 < bk->h_tables.size(); i += 2)
        if (16.0 * (fabs((double)bk->h_tables[i]) + fabs((double)bk->h_tables[i + 1])) > (double)FLT_MAX) bk->pskip_ok_i16 = false;
    *b = bk;
    return SDRHIP_OK;
}

void sdrhip_fm_bank_destroy(sdrhip_fm_bank* b) { delete b; }

int sdrhip_fm_bank_stations(const sdrhip_fm_bank* b) { return b ? (int)b->ch.size() : SDRHIP_ERR_ARG; }

int sdrhip_fm_bank_period(const sdrhip_fm_bank* b, int station)
{
    SDRHIP_REQUIRE(b != nullptr && station >= 0 && station < (int)b->ch.size(), "sdrhip_fm_bank_period");
    return b->period[station];
}

int sdrhip_fm_bank_plan(const sdrhip_fm_bank* b, int64_t s0, int64_t s1, int64_t total_in, int64_t* q0, int64_t* q1, int64_t* halo)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_fm_bank_plan");
    return sdrhip_fm_chain_plan(b->ch[0], s0, s1, total_in, q0, q1, halo);
}

int64_t sdrhip_fm_bank_ready(const sdrhip_fm_bank* b, int64_t n_samples) { return b ? sdrhip_fm_chain_ready(b->ch[0], n_samples) : -1; }

int64_t sdrhip_fm_bank_max_halo(const sdrhip_fm_bank* b) { return b ? sdrhip_fm_chain_max_halo(b->ch[0]) : -1; }

size_t sdrhip_fm_bank_workspace_bytes(const sdrhip_fm_bank* b, int64_t n_in) { return b ? sdrhip_fm_chain_workspace_bytes(b->ch[0], n_in) : 0; }

int sdrhip_fm_bank_set_route(sdrhip_fm_bank* b, int route, int64_t max_outputs, int tile_outputs)
{
    SDRHIP_REQUIRE(b != nullptr && route >= 0 && route <= 2 && max_outputs >= 0 && tile_outputs >= 0, "sdrhip_fm_bank_set_route");
    b->route = route;
    b->max_outputs = max_outputs > 0 ? max_outputs : kBankAutoOutputs;
    b->tile = tile_outputs;
    return SDRHIP_OK;
}

long long sdrhip_debug_fm_bank_launches(void) { return fm_chain_small_bank_launch_count(); }
long long sdrhip_debug_fm_bank_i16_launches(void) { return fm_chain_small_bank_i16_launch_count(); }

}  // extern "C"

// One run of a bank; sdrhip_fm_bank_run and the submissions of a bank's host-block stream.  input_over_link: as chain_run_on --
// d_in_iq is pinned HOST memory, so the one-kernel chain takes its largest tile on either route (a tile_outputs beyond the
// kernel's largest is clamped to it by the launcher; a negative one would mean "chosen from the work" to the banked launcher).
// fmt: IN_U8, or IN_I16 for sdrhip_fm_bank_run_i16 (d_in_iq: interleaved int16, 4 bytes per sample): the same object, plan and
// workspace; the banked launch is the kernel's int16 form under int16's alignment rule and its own skip predicate, and the
// stations' own runs take the tuner's int16 first stage (chain_run_on).
static int bank_run(sdrhip_fm_bank* b, void* stream, const uint8_t* d_in_iq, int64_t s0, int64_t n_in, float* d_audio, int64_t audio_stride,
                    int64_t q0, int64_t q1, void* d_workspace, size_t workspace_bytes, bool input_over_link, InFmt fmt = IN_U8)
{
    SDRHIP_REQUIRE(b != nullptr, "sdrhip_fm_bank_run");
    SDRHIP_REQUIRE(q1 >= q0 && q0 >= 0 && s0 >= 0 && n_in >= 0, "sdrhip_fm_bank_run");
    SDRHIP_REQUIRE(audio_stride >= q1 - q0, "sdrhip_fm_bank_run: a station's row holds its outputs");
    if (q1 == q0) return SDRHIP_OK;
    SDRHIP_REQUIRE(d_in_iq && d_audio, "sdrhip_fm_bank_run");
    SDRHIP_REQUIRE(fmt != IN_I16 || (reinterpret_cast<uintptr_t>(d_in_iq) & 3) == 0, "sdrhip_fm_bank_run_i16: int16 IQ at an address that is no multiple of 4");
    hipStream_t s = (hipStream_t)stream;
    const int K = (int)b->ch.size();
    sdrhip_fm_chain* c0 = b->ch[0];         // ranges, taps and tail tables are the same for every station

    // the receptive field of [q0, q1) does not depend on a table: checked once, before either route launches anything
    int rc;
    if ((rc = input_holds("sdrhip_fm_bank_run", plan_run(c0, s0, q0, q1, d_in_iq, d_workspace), s0, n_in, q0, q1)) != SDRHIP_OK) return rc;
    const int tile = b->tile != 0 ? b->tile : (input_over_link ? 1 << 20 : 0);
    const bool fits = (fmt == IN_I16 ? c0->fm_tail && fm_chain_small_i16_fits(c0->decim.factor, c0->decim.Lp, c0->decim.corder, c0->block, d_in_iq, s0)
                                     : chain_small_fits(c0, d_in_iq, s0)) &&
                      fm_chain_small_bank_fits(q0, q1, K, tile);
    if (b->route == 1 && !fits) {
        set_error("sdrhip_fm_bank_run: the banked launch does not fit this run (decimator / tail shape, seam block, input alignment, "
                  "s0 %% %d, or more than 65535 tiles)", fmt == IN_I16 ? 4 : 8);
        return SDRHIP_ERR_ARG;
    }
    const bool banked = fits && (b->route == 1 || (b->route == 0 && (int64_t)K * (q1 - q0) <= b->max_outputs && q1 - q0 <= kBankAutoStationOutputs));
    if (banked) {
        const FirDesc& dec = c0->decim;
        if ((rc = dec.ensure_device()) != SDRHIP_OK || (rc = c0->resamp.ensure_device()) != SDRHIP_OK || (rc = c0->audio.ensure_device()) != SDRHIP_OK)
            return rc;
        if (b->d_tables == nullptr && (rc = upload_floats(&b->d_tables, b->h_tables)) != SDRHIP_OK) return rc;
        if (fmt == IN_I16)
            launch_fm_chain_small_bank_i16(s, reinterpret_cast<const int16_t*>(d_in_iq), s0, n_in, d_audio, audio_stride, q0, q1, dec.d_plain,
                                           dec.last_tap_is_padding() && b->pskip_ok() && b->pskip_ok_i16, c0->tail_tables(), tile, b->d_tables, K,
                                           b->off, b->period);
        else
            launch_fm_chain_small_bank(s, d_in_iq, s0, n_in, d_audio, audio_stride, q0, q1, dec.d_plain, dec.last_tap_is_padding() && b->pskip_ok(),
                                       c0->tail_tables(), tile, b->d_tables, K, b->off, b->period);
        return launched(SDRHIP_OK);
    }
    // station by station.  What a station's run would refuse is found for ALL stations first (chain_route, the chain's own
    // refusals), so that a refused bank run has written no row: whether a tuned run takes the tuner's tile kernel, and with it the
    // workspace it needs, depends on its period
    for (int j = 0; j < K; j++) {
        RunRoute route;
        if ((rc = chain_route(b->ch[j], "sdrhip_fm_bank_run", d_in_iq, s0, n_in, d_audio, q0, q1, d_workspace, workspace_bytes, &route, fmt)) != SDRHIP_OK)
            return rc;
    }
    for (int j = 0; j < K; j++)
        if ((rc = chain_run(b->ch[j], stream, d_in_iq, s0, n_in, d_audio + (int64_t)j * audio_stride, q0, q1, d_workspace, workspace_bytes,
                            input_over_link, fmt)) != SDRHIP_OK)
            return rc;
    return SDRHIP_OK;
}

extern "C" {

int sdrhip_fm_bank_run(sdrhip_fm_bank* b, void* stream, const uint8_t* d_in_iq, int64_t s0, int64_t n_in, float* d_audio, int64_t audio_stride,
                       int64_t q0, int64_t q1, void* d_workspace, size_t workspace_bytes)
{
    return bank_run(b, stream, d_in_iq, s0, n_in, d_audio, audio_stride, q0, q1, d_workspace, workspace_bytes, false);
}

int sdrhip_fm_bank_run_i16(sdrhip_fm_bank* b, void* stream, const int16_t* d_in_iq, int64_t s0, int64_t n_in, float* d_audio, int64_t audio_stride,
                           int64_t q0, int64_t q1, void* d_workspace, size_t workspace_bytes)
{
    return bank_run(b, stream, reinterpret_cast<const uint8_t*>(d_in_iq), s0, n_in, d_audio, audio_stride, q0, q1, d_workspace, workspace_bytes, false,
                    IN_I16);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Host-block streaming front end of the chain: what a Haskell `Pipe (Vector CUChar) (Vector Float)`
// replacing the five middle stages of examples/fm/fm.hs:34-41 binds to.  Source blocks (u8 IQ, host
// memory, `block` samples each -- or a multiple) go in, audio blocks of exactly `block_size_out`
// floats come out, bit-identical to what the reference's four Pipes + convert + gain yield.
//
// Slots, staging, the carried tail (~4.4k samples, 8 KB copied by the host) and the three submission routes are the
// host-block engine's (host_stream.hpp).  This operator picks the route by the size of [carried tail | staged samples]:
//   * large submissions (> direct_samples): the copy engines -- upload of block i over compute of i-1 over download of i-2;
//   * from stage_samples up: one copy into device memory on the slot's own compute stream, then the chain on device memory;
//   * a lone source block: NO copies at all -- the decimator kernel reads the pinned host buffer directly over PCIe and the
//     last kernel writes the audio straight into pinned host memory: ONE kernel launch for a push of a few blocks
//     (kernels_small.hip; two launches -- decimator with its seams, fused tail -- where the one-kernel chain does not apply)
//     and one event per push instead of ~15 API calls, which is what the reference's own block size (8192 samples) needs to
//     beat one CPU thread.
// Results lag at most nslots - 1 submissions (sdrhip_fm_stream_flush drains); with adaptive submission (the default for
// operators that run in place) a push that finds the next slot still busy is staged behind the earlier ones and leaves with them.
//
// The same stream serves a receiver bank (sdrhip_fm_stream_create_bank): rows = the bank's stations.  Position, carried tail,
// slots, adaptive cap and knobs are the chain stream's -- they depend on no table -- and three things differ: a submission is ONE
// run of the bank (bank_run: the banked launch or station by station, by the bank's own rule) writing its rows back to back into
// the slot's result buffer; the engine's harvest regroups them into one fifo per station; and a stream of several rows never
// runs in place (stream_create says why).
// ---------------------------------------------------------------------------
// Round 5: the caller-side copy of a LARGE push into the pinned staging buffer, split over a few threads.  A push of 4096 source
// blocks is a 64 MiB memcpy: one thread moves ~23 GB/s while the link behind it takes ~45 (profiles/r04_host_stream.txt: 11.4
// against 22.5 Gsample/s with the source writing the staging buffer itself) -- the copying push lost half the link to a
// single-threaded memcpy.  Helpers are started by the first large push and live as long as the operator; the caller copies its
// own share, so small pushes never touch them (SDRHIP_COPY_THREADS: helpers, default 3; 0 = plain memcpy).
namespace {
struct CopyPool {
    static constexpr size_t kMinBytes = 4u << 20;          // below this a push is one memcpy
    static constexpr size_t kPiece = 1u << 20;
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    uint8_t* dst = nullptr;
    const uint8_t* src = nullptr;
    size_t bytes = 0;
    std::atomic<size_t> next{0};
    int generation = 0, active = 0;
    bool stop = false;
    // helper threads beside the caller's own (SDRHIP_COPY_THREADS, clamped to 0 .. 16; 0 = plain memcpy)
    int helpers = [] {
        const char* e = getenv("SDRHIP_COPY_THREADS");
        const long v = e ? strtol(e, nullptr, 10) : 3;
        return (int)(v < 0 ? 0 : v > 16 ? 16 : v);
    }();

    void drain()
    {
        for (;;) {
            const size_t o = next.fetch_add(kPiece, std::memory_order_relaxed);
            if (o >= bytes) return;
            memcpy(dst + o, src + o, bytes - o < kPiece ? bytes - o : kPiece);
        }
    }
    void worker()
    {
        int seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv_job.wait(lk, [&] { return stop || generation != seen; });
            if (stop) return;
            seen = generation;
            lk.unlock();
            drain();
            lk.lock();
            if (--active == 0) cv_done.notify_one();
        }
    }
    void copy(uint8_t* d, const uint8_t* s, size_t n)
    {
        if (n < kMinBytes || helpers <= 0) {
            memcpy(d, s, n);
            return;
        }
        if (workers.empty()) {
            // a thread that cannot be started (std::system_error: resource limits) must not unwind through the extern "C" push: the
            // copy goes on with the helpers that did start, or as a plain memcpy
            try {
                for (int i = 0; i < helpers; i++) workers.emplace_back([this] { worker(); });
            } catch (const std::exception&) {
                helpers = (int)workers.size();
            }
            if (workers.empty()) {
                helpers = 0;
                memcpy(d, s, n);
                return;
            }
        }
        {
            std::lock_guard<std::mutex> lk(m);
            dst = d; src = s; bytes = n;
            next.store(0, std::memory_order_relaxed);
            active = (int)workers.size();
            generation++;
        }
        cv_job.notify_all();
        drain();                                            // the caller's own share
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return active == 0; });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv_job.notify_all();
        for (auto& t : workers) t.join();
    }
};
}  // namespace

struct sdrhip_fm_stream {
    sdrhip_fm_chain* c = nullptr;        // a bank's stream: station 0's chain -- positions, ranges and sizes depend on no table
    sdrhip_fm_bank* bank = nullptr;      // set: every submission is ONE run of the bank, rows = its stations
    int rows = 1;
    // what is pushed: u8 IQ (2 bytes per sample) or, over a bank only (sdrhip_fm_stream_create_bank_i16), interleaved int16 IQ
    // (4 bytes per sample): staging, history and states hold the samples as they came
    InFmt fmt = IN_U8;
    size_t esz() const { return (size_t)in_fmt_bytes(fmt); }
    CopyPool copier;
    int max_block = 0;
    int block_out = 0;
    // Slots: submissions in flight.  Two for operators that take large pushes (upload of block i over compute of i-1 over
    // download of i-2, each slot holding a pinned staging buffer of the largest push); FOUR for operators whose largest push
    // runs in place (round 3): such a push is one small kernel, i.e. ~20 us of latency end to end over PCIe, and the host is
    // done submitting it in ~6 -- the slots are what keeps the GPU fed.  Results then lag three pushes instead of one
    // (sdrhip_fm_stream_flush drains; SDRHIP_STREAM_SLOTS=2 restores the short lag).
    DevBuf ws[HostStream::kMaxSlots];    // one workspace per compute stream
    int64_t N = 0;         // samples received so far
    int64_t q_done = 0;    // audio outputs computed so far
    bool direct_ok = stream_knobs().direct;
    // [tail | new] up to this many samples is read in place over PCIe (tunable for experiments: SDRHIP_DIRECT_SAMPLES)
    int64_t direct_samples = getenv("SDRHIP_DIRECT_SAMPLES") ? atoll(getenv("SDRHIP_DIRECT_SAMPLES")) : kDirectSamples;
    // round 6 (tools/stream_direct_threshold_probe.py, after the in-place pushes got the largest tile): in place 11.1 / 11.7 / 12.2 Gsample/s
    // at 48 / 64 / 96 blocks per push against 8.2 / 10.5 / 13.4 through the copy engines (zero-copy pushes; memcpy pushes cross at ~110 blocks)
    // ... and with the slot-stream staging copy (below) 19-24 Gsample/s from 2 to 160 blocks per push against 13-17 through the three-stream
    // copy path at 96 ... 128 blocks; the two meet at ~256 blocks (21.7 either way)
    static constexpr int64_t kDirectSamples = 200 * 8192;
    // pushes (or piled-up batches) of at least this many samples are copied to device memory on their slot's stream before the chain runs
    int64_t stage_samples = getenv("SDRHIP_STAGE_SAMPLES") ? atoll(getenv("SDRHIP_STAGE_SAMPLES")) : 2 * 8192;
    int coalesce = 0;          // submit once this many samples are staged (0: every push)
    int adaptive = 0;          // > 0: submit when the next slot is free, else keep staging up to this many samples
    int capacity() const
    {
        int c = coalesce > max_block ? coalesce : max_block;
        return adaptive > c ? adaptive : c;
    }
    int ready() const { return (int)(eng.pending() / (size_t)block_out); }
    // u8 IQ samples (2 bytes) or int16 IQ samples (4 bytes: esz()); head room = the carried tail, a multiple of 8 samples.  Declared last: destroyed first, so its
    // streams are idle before the workspaces are freed.
    HostStream eng;
};

// A stream over a chain (bank == nullptr, one row) or over a bank (chain: its station 0); the arguments are checked by the callers
static int stream_create(const char* who, sdrhip_fm_stream** out, sdrhip_fm_chain* chain, sdrhip_fm_bank* bank, int max_block_samples,
                         int block_size_out, InFmt fmt = IN_U8)
{
    *out = nullptr;
    sdrhip_fm_stream* st = new sdrhip_fm_stream();
    st->c = chain;
    st->bank = bank;
    st->fmt = fmt;
    st->rows = bank ? (int)bank->ch.size() : 1;
    st->eng.set_rows(st->rows);
    // More than one row never runs in place: with K stations in the grid every station's workgroups would fetch the same tile
    // over the link.  tools/fm_bank_stream_bench.py (profiles/fm_bank_stream_bench.txt), lone-block pushes at 2 / 4 / 8 / 12
    // stations: in place has the lower medians (4.2 .. 4.7 against 5.9 .. 8.8 us per push) but is at no K ahead of the copy by
    // more than the spread of the rounds, which is what an in-place region would have needed -- none is kept.
    // SDRHIP_STAGE_SAMPLES still moves the bound, for that comparison.
    if (st->rows > 1 && getenv("SDRHIP_STAGE_SAMPLES") == nullptr) st->stage_samples = 0;
    // An int16 stream never reads its input in place, whatever the station count and whatever the knob says: a stated choice, not a
    // measured one (for K >= 2 it is the rule above; for K = 1 it differs from the u8 stream's).  The carried tail starts at a
    // multiple of 8 samples, so the copy puts the run's first sample on a 16-byte boundary of the slot's device buffer.
    if (fmt == IN_I16) st->stage_samples = 0;
    st->max_block = max_block_samples;
    st->block_out = block_size_out;
    // the carried tail never exceeds the receptive field of one audio output (+ the 8-sample alignment of its start)
    const int64_t head_cap = (sdrhip_fm_chain_max_halo(chain) + 8 + 15) / 8 * 8;
    // four slots when even the largest push runs in place (see the struct), else two
    const int slots = (st->direct_ok && head_cap + (int64_t)max_block_samples <= st->direct_samples) ? HostStream::kMaxSlots : 2;
    if (st->eng.init(slots, st->esz(), head_cap, who) != SDRHIP_OK) {
        delete st;
        return SDRHIP_ERR_HIP;
    }
    // adaptive submission by default for operators that run in place (sdrhip_fm_stream_set_adaptive; SDRHIP_STREAM_ADAPTIVE=0
    // switches the default off, =n caps it at n source blocks): up to what is still read in place over PCIe
    if (st->eng.nslots == HostStream::kMaxSlots) {
        const std::optional<int64_t>& env = stream_knobs().adaptive;
        const int64_t unit = chain->block > 0 ? chain->block : 8;
        int64_t cap = (st->direct_samples - head_cap) / unit;
        // ... but no more than 64 source blocks' worth (or two of the caller's largest pushes): the one-stream route is within 10 % of its full rate
        // with batches of that size (32: 13-15, 64: 18-21, 199: 20-22 Gsample/s), and what piles up beyond only adds to the push-to-audio lag
        const int64_t enough = std::max<int64_t>((64 * (int64_t)8192 + unit - 1) / unit, 2 * (((int64_t)max_block_samples + unit - 1) / unit));
        if (cap > enough) cap = enough;
        if (env && *env < cap) cap = *env;
        cap *= unit;
        if (cap >= 2 * (int64_t)max_block_samples && cap <= (1 << 30)) st->adaptive = (int)cap;
    }
    *out = st;
    return SDRHIP_OK;
}

extern "C" {

int sdrhip_fm_stream_create(sdrhip_fm_stream** out, sdrhip_fm_chain* chain, int max_block_samples, int block_size_out)
{
    SDRHIP_REQUIRE(out != nullptr && chain != nullptr && max_block_samples > 0 && block_size_out > 0, "sdrhip_fm_stream_create");
    SDRHIP_REQUIRE(chain->block == 0 || max_block_samples % chain->block == 0,
                   "sdrhip_fm_stream_create: blocks must be whole multiples of the chain's seam block");
    return stream_create("sdrhip_fm_stream_create", out, chain, nullptr, max_block_samples, block_size_out);
}

int sdrhip_fm_stream_create_bank(sdrhip_fm_stream** out, sdrhip_fm_bank* bank, int max_block_samples, int block_size_out)
{
    SDRHIP_REQUIRE(out != nullptr && bank != nullptr && max_block_samples > 0 && block_size_out > 0, "sdrhip_fm_stream_create_bank");
    SDRHIP_REQUIRE(bank->ch[0]->block == 0 || max_block_samples % bank->ch[0]->block == 0,
                   "sdrhip_fm_stream_create_bank: blocks must be whole multiples of the bank's seam block");
    return stream_create("sdrhip_fm_stream_create_bank", out, bank->ch[0], bank, max_block_samples, block_size_out);
}

int sdrhip_fm_stream_create_bank_i16(sdrhip_fm_stream** out, sdrhip_fm_bank* bank, int max_block_samples, int block_size_out)
{
    SDRHIP_REQUIRE(out != nullptr && bank != nullptr && max_block_samples > 0 && block_size_out > 0, "sdrhip_fm_stream_create_bank_i16");
    SDRHIP_REQUIRE(bank->ch[0]->block == 0 || max_block_samples % bank->ch[0]->block == 0,
                   "sdrhip_fm_stream_create_bank_i16: blocks must be whole multiples of the bank's seam block");
    return stream_create("sdrhip_fm_stream_create_bank_i16", out, bank->ch[0], bank, max_block_samples, block_size_out, IN_I16);
}

int sdrhip_fm_stream_rows(const sdrhip_fm_stream* st)
{
    SDRHIP_REQUIRE(st != nullptr, "sdrhip_fm_stream_rows");
    return st->rows;
}

void sdrhip_fm_stream_destroy(sdrhip_fm_stream* st) { delete st; }

}  // extern "C"


// Submit everything staged in the current slot: [carried tail | staged samples] -> chain -> audio -> host.
static int stream_submit(sdrhip_fm_stream* st)
{
    sdrhip_fm_chain* c = st->c;
    HostStream& e = st->eng;
    const int n = e.staged;
    if (n == 0) return SDRHIP_OK;
    const int si = e.cur();
    int rc;
    // outputs whose receptive field is complete once these samples are in
    const int64_t N1 = st->N + n;
    int64_t q_new = sdrhip_fm_chain_ready(c, N1);
    if (q_new < st->q_done) q_new = st->q_done;
    // the tail starts at the first sample the next pending output needs, rounded down to a multiple of 8 samples
    // (16-byte aligned tiles for the LDS-tiled decimator; tail and head_cap are multiples of 8 samples)
    int64_t keep_from = c->start(st->q_done) & ~(int64_t)7;
    if (keep_from > st->N) keep_from = st->N & ~(int64_t)7;
    const int64_t tail = st->N - keep_from;
    const uint8_t* first = e.carry(keep_from, st->N, n, "sdrhip_fm_stream");
    if (first == nullptr) return SDRHIP_ERR_STATE;

    const int64_t n_out = q_new - st->q_done;
    const bool direct = st->direct_ok && tail + n <= st->direct_samples;
    // In-place pushes alternate between the slots' compute streams (and workspaces): a push of one source block is a few small
    // kernels, i.e. latency, and nothing push i+1 computes depends on what push i left on the device (the carried tail
    // comes from the host-side history) -- so consecutive pushes overlap on the GPU.
    hipStream_t cs = direct ? e.compute[si] : e.compute[0];
    DevBuf& wsb_buf = direct ? st->ws[si] : st->ws[0];
    if (n_out > 0) {
        const size_t wsb = sdrhip_fm_chain_workspace_bytes(c, tail + n);
        if (wsb > wsb_buf.cap) {
            // growing frees the old buffer: nothing may still be using it
            SDRHIP_CHECK_HIP(hipStreamSynchronize(cs));
        }
        if ((rc = wsb_buf.ensure(wsb)) != SDRHIP_OK) return rc;
    }
    // From stage_samples up, ONE pass over the link into device memory on the slot's own compute stream, then the chain on device
    // memory (round 6): read in place, the one-kernel chain fetches every sample ~1.95 times over PCIe (each tile re-reads its
    // overlap), and the link is what such a push costs -- 8 ... 64 blocks per push 10-11 -> 19-24 Gsample/s.  A lone source block
    // (a paced real-time source: the GPU is idle when it arrives) is read in place by the kernel itself.
    const HostStream::Route route = !direct ? HostStream::kCopyEngines
                                  : tail + n >= st->stage_samples ? HostStream::kSlotStream : HostStream::kInPlace;
    // A bank's stream: ONE run of the bank on the same [tail | staged], its rows back to back in the result buffer (the engine's
    // harvest regroups them per station).  The bank's own rule picks the banked launch or station by station, on the same
    // workspace: sdrhip_fm_bank_workspace_bytes is the chain's figure.
    rc = e.submit(route, cs, first, (size_t)(tail + n) * st->esz(), (int64_t)st->rows * n_out, [&](hipStream_t s, const void* d_in, void* d_out) {
        if (st->bank)
            return bank_run(st->bank, (void*)s, (const uint8_t*)d_in, keep_from, tail + n, (float*)d_out, n_out, st->q_done, q_new, wsb_buf.p,
                            wsb_buf.cap, route == HostStream::kInPlace, st->fmt);
        return chain_run(c, (void*)s, (const uint8_t*)d_in, keep_from, tail + n, (float*)d_out, st->q_done, q_new, wsb_buf.p, wsb_buf.cap,
                         route == HostStream::kInPlace);
    });
    if (rc != SDRHIP_OK) return rc;
    st->q_done = q_new;
    st->N = N1;
    return SDRHIP_OK;
}

extern "C" {

int sdrhip_fm_stream_set_coalesce(sdrhip_fm_stream* st, int samples)
{
    SDRHIP_REQUIRE(st != nullptr && samples >= 0, "sdrhip_fm_stream_set_coalesce");
    SDRHIP_REQUIRE(st->eng.staged == 0, "sdrhip_fm_stream_set_coalesce: samples are staged (flush first)");
    SDRHIP_REQUIRE(st->c->block == 0 || samples % st->c->block == 0, "sdrhip_fm_stream_set_coalesce: whole source blocks only");
    int rc = st->eng.sync();   // staging buffers may be reallocated
    if (rc != SDRHIP_OK) return rc;
    st->coalesce = samples;
    return SDRHIP_OK;
}

int sdrhip_fm_stream_set_adaptive(sdrhip_fm_stream* st, int max_samples)
{
    SDRHIP_REQUIRE(st != nullptr && max_samples >= 0, "sdrhip_fm_stream_set_adaptive");
    SDRHIP_REQUIRE(st->eng.staged == 0, "sdrhip_fm_stream_set_adaptive: samples are staged (flush first)");
    SDRHIP_REQUIRE(st->c->block == 0 || max_samples % st->c->block == 0, "sdrhip_fm_stream_set_adaptive: whole source blocks only");
    SDRHIP_REQUIRE(max_samples == 0 || max_samples >= 2 * st->max_block, "sdrhip_fm_stream_set_adaptive: room for at least two pushes");
    int rc = st->eng.sync();   // staging buffers may be reallocated
    if (rc != SDRHIP_OK) return rc;
    st->adaptive = max_samples;
    return SDRHIP_OK;
}

}  // extern "C"

// the wrong push / input_buffer call for the stream's input type is refused with nothing staged
static const char* stream_wrong_type(const sdrhip_fm_stream* st, InFmt fmt)
{
    if (st->fmt == fmt) return nullptr;
    return st->fmt == IN_I16 ? "this stream takes int16 IQ (sdrhip_fm_stream_push_i16 / sdrhip_fm_stream_input_buffer_i16)"
                             : "this stream takes u8 IQ (sdrhip_fm_stream_push / sdrhip_fm_stream_input_buffer)";
}

static uint8_t* stream_input_buffer(sdrhip_fm_stream* st, InFmt fmt, const char* who)
{
    if (st == nullptr) { set_error("%s: null stream", who); return nullptr; }
    if (const char* wrong = stream_wrong_type(st, fmt)) { set_error("%s: %s", who, wrong); return nullptr; }
    HostStream& e = st->eng;
    // the caller may write up to max_block samples: make room for all of them behind what is already staged
    if (e.staged + st->max_block > st->capacity() && stream_submit(st) != SDRHIP_OK) return nullptr;
    if (e.open_slot((size_t)st->capacity() * st->esz(), (size_t)e.staged * st->esz()) != SDRHIP_OK) return nullptr;
    return e.write_pos();
}

static int stream_push(sdrhip_fm_stream* st, const void* iq_v, int n, InFmt fmt, const char* who)
{
    SDRHIP_REQUIRE(st != nullptr && iq_v != nullptr && n > 0 && n <= st->max_block, who);
    if (const char* wrong = stream_wrong_type(st, fmt)) {
        set_error("%s: %s", who, wrong);
        return SDRHIP_ERR_ARG;
    }
    SDRHIP_REQUIRE(st->c->block == 0 || n % st->c->block == 0,
                   "sdrhip_fm_stream_push: the chain reproduces the seams of `block`-sample source buffers (fm.hs:17,24)");
    const uint8_t* iq = static_cast<const uint8_t*>(iq_v);
    HostStream& e = st->eng;
    int rc;
    if (e.staged + n > st->capacity() && (rc = stream_submit(st)) != SDRHIP_OK) return rc;
    if ((rc = e.open_slot((size_t)st->capacity() * st->esz(), (size_t)e.staged * st->esz())) != SDRHIP_OK) return rc;
    uint8_t* dst = e.write_pos();
    if (iq != dst) st->copier.copy(dst, iq, (size_t)n * st->esz());   // else: the caller filled our staging buffer in place
    e.staged += n;
    bool submit = e.staged >= st->coalesce;
    if (st->adaptive > 0 && st->coalesce == 0 && submit) {     // an explicit set_coalesce takes precedence: fixed batches
        // a GPU that keeps up gets every push at once (lowest latency); one that is still busy with the slot this submission
        // would move on to lets the pushes pile up in the staging buffer and takes them as ONE launch when it frees up
        const bool room = e.staged + st->max_block <= st->capacity();
        submit = !room || !e.next_in_flight();
    }
    if (submit) {
        if ((rc = stream_submit(st)) != SDRHIP_OK) return rc;
        // a push that went out also collects whatever the GPU has finished meanwhile: a source slower than the GPU gets the
        // audio of push i at push i + 1 instead of i + nslots - 1 (staged pushes skip the query)
        if ((rc = e.harvest_done()) != SDRHIP_OK) return rc;
    }
    return st->ready();
}

extern "C" {

uint8_t* sdrhip_fm_stream_input_buffer(sdrhip_fm_stream* st) { return stream_input_buffer(st, IN_U8, "sdrhip_fm_stream_input_buffer"); }

int16_t* sdrhip_fm_stream_input_buffer_i16(sdrhip_fm_stream* st)
{
    return reinterpret_cast<int16_t*>(stream_input_buffer(st, IN_I16, "sdrhip_fm_stream_input_buffer_i16"));
}

int sdrhip_fm_stream_push(sdrhip_fm_stream* st, const uint8_t* iq, int n) { return stream_push(st, iq, n, IN_U8, "sdrhip_fm_stream_push"); }

int sdrhip_fm_stream_push_i16(sdrhip_fm_stream* st, const int16_t* iq, int n_samples)
{
    return stream_push(st, iq, n_samples, IN_I16, "sdrhip_fm_stream_push_i16");
}

int sdrhip_fm_stream_poll(sdrhip_fm_stream* st)
{
    SDRHIP_REQUIRE(st != nullptr, "sdrhip_fm_stream_poll");
    int rc = st->eng.harvest_done();
    if (rc != SDRHIP_OK) return rc;
    return st->ready();
}

int sdrhip_fm_stream_flush(sdrhip_fm_stream* st)
{
    SDRHIP_REQUIRE(st != nullptr, "sdrhip_fm_stream_flush");
    int rc;
    if ((rc = stream_submit(st)) != SDRHIP_OK || (rc = st->eng.flush()) != SDRHIP_OK) return rc;
    return st->ready();
}

// ---- checkpoint / resume ------------------------------------------------------------------------
// The whole state of the operator between two pushes is small and explicit (the reference keeps it in Pipe
// closures -- overlap remainder, resampler phase, last demod sample, output fill level): the stream position, the number of
// audio samples produced, the last head_cap input samples, and the audio not yet popped.  Everything else (resampler group,
// demod history, seam positions) is a closed form of the position.
namespace {
struct StreamStateHeader {
    uint32_t magic, version;
    int64_t N, q_done, head_cap, hist_n, pending;   // pending: audio floats in the fifo
    int32_t block_out, chain_block;
    int64_t chain_halo;
};
constexpr uint32_t kStateMagic = 0x53444d46u;   // "FMDS"
// A stream of one row writes version 1, byte for byte what it always wrote.  A stream of several rows (over a bank) writes
// version 2: the same header with `pending` counted PER ROW, then the row count (int64), then the history and every row's audio
// not yet popped, row after row.  Oscillator tables are no part of a state: a station's phase is a closed form of the position.
// An int16 stream writes version 3 whatever its row count: version 2's layout (the row count is always there) with the history as
// int16 IQ, 4 bytes per sample.  The version IS the input type: restore refuses a version 3 state on a u8 stream and the reverse.
size_t state_header_bytes(const sdrhip_fm_stream* st)
{
    return sizeof(StreamStateHeader) + (st->rows > 1 || st->fmt == IN_I16 ? sizeof(int64_t) : 0);
}
}  // namespace

size_t sdrhip_fm_stream_state_bytes(sdrhip_fm_stream* st)
{
    if (st == nullptr) return 0;
    // exact: drains the operator exactly as sdrhip_fm_stream_save will (0 = the drain failed, sdrhip_last_error)
    if (sdrhip_fm_stream_flush(st) < 0) return 0;
    return state_header_bytes(st) + st->eng.state_bytes(st->eng.hist_n, (int64_t)st->eng.pending());
}

int sdrhip_fm_stream_save(sdrhip_fm_stream* st, void* buf, size_t capacity, size_t* used)
{
    SDRHIP_REQUIRE(st != nullptr && buf != nullptr && used != nullptr, "sdrhip_fm_stream_save");
    int rc = sdrhip_fm_stream_flush(st);             // submits what is staged, drains every slot into the fifo
    if (rc < 0) return rc;
    StreamStateHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kStateMagic;
    h.version = st->fmt == IN_I16 ? 3 : st->rows > 1 ? 2 : 1;
    h.N = st->N;
    h.q_done = st->q_done;
    h.head_cap = st->eng.head_cap;
    h.hist_n = st->eng.hist_n;
    h.pending = (int64_t)st->eng.pending();
    h.block_out = st->block_out;
    h.chain_block = st->c->block;
    h.chain_halo = sdrhip_fm_chain_max_halo(st->c);
    const size_t need = state_header_bytes(st) + st->eng.state_bytes(h.hist_n, h.pending);
    if (capacity < need) {
        set_error("sdrhip_fm_stream_save: %zu bytes needed, %zu given", need, capacity);
        return SDRHIP_ERR_ARG;
    }
    memcpy(buf, &h, sizeof h);
    if (state_header_bytes(st) > sizeof h) {
        const int64_t rows = st->rows;
        memcpy((unsigned char*)buf + sizeof h, &rows, sizeof rows);
    }
    st->eng.save((unsigned char*)buf + state_header_bytes(st));
    *used = need;
    return SDRHIP_OK;
}

int sdrhip_fm_stream_restore(sdrhip_fm_stream* st, const void* buf, size_t bytes)
{
    SDRHIP_REQUIRE(st != nullptr && buf != nullptr && bytes >= sizeof(StreamStateHeader), "sdrhip_fm_stream_restore");
    SDRHIP_REQUIRE(st->N == 0 && st->eng.staged == 0 && st->eng.pushes == 0,
                   "sdrhip_fm_stream_restore: only into a stream that has not been pushed to");
    StreamStateHeader h;
    memcpy(&h, buf, sizeof h);
    SDRHIP_REQUIRE(h.magic == kStateMagic && h.version >= 1 && h.version <= 3, "sdrhip_fm_stream_restore: not a stream state");
    SDRHIP_REQUIRE((h.version == 3) == (st->fmt == IN_I16),
                   "sdrhip_fm_stream_restore: the state belongs to a stream of another input type (u8 / int16 IQ)");
    int64_t rows = 1;
    if (h.version >= 2) {
        SDRHIP_REQUIRE(bytes >= sizeof h + sizeof rows, "sdrhip_fm_stream_restore: truncated state");
        memcpy(&rows, (const unsigned char*)buf + sizeof h, sizeof rows);
    }
    SDRHIP_REQUIRE(rows == st->rows && (h.version == 3 || (h.version == 2) == (st->rows > 1)) && h.block_out == st->block_out && h.chain_block == st->c->block &&
                       h.head_cap == st->eng.head_cap && h.chain_halo == sdrhip_fm_chain_max_halo(st->c),
                   "sdrhip_fm_stream_restore: the state belongs to a stream of another geometry (stations / chain taps / block sizes)");
    SDRHIP_REQUIRE(h.hist_n >= 0 && h.hist_n <= h.head_cap && h.pending >= 0 && h.pending <= (int64_t)(bytes / sizeof(float)) && h.N >= h.hist_n &&
                       h.q_done >= 0,
                   "sdrhip_fm_stream_restore: inconsistent state");
    SDRHIP_REQUIRE(bytes >= state_header_bytes(st) + st->eng.state_bytes(h.hist_n, h.pending), "sdrhip_fm_stream_restore: truncated state");
    st->eng.restore((const unsigned char*)buf + state_header_bytes(st), h.hist_n, h.pending);
    st->N = h.N;
    st->q_done = h.q_done;
    return st->ready();
}

int sdrhip_fm_stream_pop(sdrhip_fm_stream* st, float* out, int capacity)
{
    SDRHIP_REQUIRE(st != nullptr && out != nullptr, "sdrhip_fm_stream_pop");
    SDRHIP_REQUIRE(st->rows == 1, "sdrhip_fm_stream_pop: a stream of several stations is popped with sdrhip_fm_stream_pop_rows");
    if (st->ready() <= 0) return 0;
    SDRHIP_REQUIRE(capacity >= st->block_out, "sdrhip_fm_stream_pop: capacity smaller than the block");
    st->eng.take((size_t)st->block_out, out);
    return st->block_out;
}

int sdrhip_fm_stream_pop_rows(sdrhip_fm_stream* st, float* out, int64_t row_stride, int max_blocks)
{
    SDRHIP_REQUIRE(st != nullptr && out != nullptr && max_blocks >= 0, "sdrhip_fm_stream_pop_rows");
    SDRHIP_REQUIRE(row_stride >= (int64_t)max_blocks * st->block_out, "sdrhip_fm_stream_pop_rows: a station's row holds max_blocks blocks");
    const int nb = st->ready() < max_blocks ? st->ready() : max_blocks;
    if (nb > 0) st->eng.take_rows((size_t)nb * (size_t)st->block_out, out, row_stride);
    return nb;
}

}  // extern "C"
