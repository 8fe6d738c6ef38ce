// pipes.cpp -- layer (3): the reference's Pipes operators on HOST blocks.
//
//   firFilter    Filter.hs:532-569      firDecimator  Filter.hs:574-611      firResampler Filter.hs:679-727
//   fmDemod      Demod.hs:40-46         amDemod       P.map (VG.map magnitude), the Readme's AM receiver
//
// The reference's state machines alternate `simple` (outputs whose window fits in the current input buffer: the C SIMD kernel) and
// `crossover` (outputs straddling two buffers: the sequential Haskell kernel), re-blocking the outputs into vectors of exactly
// blockSizeOut (advanceOutBuf, Filter.hs:516-523: a block is yielded only when exactly full).  Here each pushed block triggers at most
// two launches on the pipe's stream -- the Cross outputs straddling the boundary with the previous block, then the One outputs inside
// the new block -- over a device buffer that holds [carried tail | new block].  Block sizes may vary from push to push.
//
// Slots, staging, the carried tail (the last < Lp/I + D/I elements earlier pushes delivered and pending outputs still need)
// and the submission routes are the host-block engine's (host_stream.hpp).  Submissions of up to kDirectBytes of input run
// in place: the kernels read the pinned staging buffer and write the pinned result buffer directly over PCIe, which leaves one
// kernel launch (seams decided inside it) and one event per push -- the reference's own block sizes (8192 .. 65536 elements)
// are launch-bound, not bandwidth-bound.  Larger ones go through the copy engines (upload of i over compute of i-1 over
// download of i-2).  Up to four submissions are in flight, so results lag up to three pushes; sdrhip_pipe_flush() drains.
//
// The tuner bank's Pipe (sdrhip_pipe_tuner_bank) is the tuner's Pipe with the engine's rows: one submission computes every
// channel's outputs into a row-major chunk which the harvest regroups into one fifo per channel.  Its blocks may be u8 IQ (2 bytes
// per element from the staging buffer to the kernels' loaders) or int16 IQ (4 bytes per element, sdrhip_pipe_tuner_bank_i16).  With
// more than one row nothing is read in place: up to kDirectBytes a submission is one copy on the slot's stream and the launch behind
// it, placed in device memory so that the banked launch's first window is 16-byte aligned (HostStream::dev_skew).
//
// The waterfall Pipe (sdrhip_pipe_spectrum), the spectrum operator's reducing form on the same engine: pipes_spectrum.cpp.
#include "deemph.hpp"
#include "pipe.hpp"

int pipe_new(sdrhip_pipe** out, PipeKind kind, const FirDesc* fir, const ResampDesc* rs, int block_out, bool cplx_in, bool cplx_out, int I,
             int D, int Lp, InFmt fmt, int64_t head_cap)
{
    sdrhip_pipe* p = new sdrhip_pipe();
    p->kind = kind; p->fir = fir; p->rs = rs; p->block_out = block_out;
    p->cplx_in = cplx_in; p->cplx_out = cplx_out; p->fmt = fmt;
    p->I = I; p->D = D; p->Lp = Lp;
    if (head_cap < 0 && p->is_map()) head_cap = 0;
    if (head_cap < 0) {
        const int64_t max_tail = ((int64_t)Lp + D) / I + 2;
        const int64_t a = p->tail_align();                  // (4: the figures every float pipe always had)
        head_cap = (max_tail + (a - 1) + (a - 1)) / a * a + a;
    }
    int rc = p->eng.init(HostStream::kMaxSlots, p->ein(), head_cap, "pipe: stream/event creation failed");
    if (rc != SDRHIP_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return SDRHIP_OK;
}

int ready_blocks(const sdrhip_pipe* p)
{
    if (p->is_map()) {
        // complete blocks = those whose floats have all been harvested
        size_t have = p->eng.pending(), n = 0;
        for (int blk : p->demod_blocks) {
            const size_t len = (size_t)blk * p->esz_out();
            if (have < len) break;
            have -= len;
            n++;
        }
        return (int)n;
    }
    return (int)(p->eng.pending() / ((size_t)p->block_out * p->esz_out()));
}

int pipe_dev_state(sdrhip_pipe** pp, DevBuf& buf, size_t bytes, const void* init, const char* who)
{
    sdrhip_pipe* p = *pp;
    int rc = buf.ensure(bytes < 16 ? 16 : bytes);
    if (rc == SDRHIP_OK) {
        hipError_t e = init ? hipMemcpy(buf.p, init, bytes, hipMemcpyHostToDevice) : hipMemsetAsync(buf.p, 0, bytes, p->eng.compute[0]);
        if (e == hipSuccess) return SDRHIP_OK;
        set_error("%s: %s", who, hipGetErrorString(e));
        rc = SDRHIP_ERR_HIP;
    }
    delete p;
    *pp = nullptr;
    return rc;
}

extern "C" {

int sdrhip_pipe_fir_filter(sdrhip_pipe** pp, const sdrhip_filter* f, int block_size_out)
{
    SDRHIP_REQUIRE(pp && f && block_size_out > 0, "sdrhip_pipe_fir_filter");
    return pipe_new(pp, PK_FILTER, f, nullptr, block_size_out, f->cplx, f->cplx, 1, 1, f->Lp);
}

int sdrhip_pipe_fir_decimator(sdrhip_pipe** pp, const sdrhip_decimator* d, int block_size_out)
{
    SDRHIP_REQUIRE(pp && d && block_size_out > 0, "sdrhip_pipe_fir_decimator");
    return pipe_new(pp, PK_DECIMATOR, d, nullptr, block_size_out, d->cplx, d->cplx, 1, d->factor, d->Lp);
}

int sdrhip_pipe_tuner(sdrhip_pipe** pp, const sdrhip_tuner* t, int block_size_out)
{
    SDRHIP_REQUIRE(pp && t && block_size_out > 0, "sdrhip_pipe_tuner");
    int rc = pipe_new(pp, PK_TUNER, &t->fir, nullptr, block_size_out, true, true, 1, t->fir.factor, t->fir.Lp);
    if (rc == SDRHIP_OK) (*pp)->tuner = t;
    return rc;
}

// The four bank Pipes: the checks (all of them before pipe_new, whose engine creates streams: a refused create has done no device
// work), the pipe with one engine row per channel, its policy (PipePolicy, pipe.hpp), and the form's state on the device, one pair of
// floats per channel, zeroed: nstate 1 = dcBlocker's pairs (dc; func 0 0, Filter.hs:731), 2 = fmDemod's in ping-pong (fm; every channel
// starts from (0, 0), Demod.hs:41).  max_type: the last input type the call takes (1: sdrhip_pipe_tuner_bank's input_u8).
static int bank_pipe_new(sdrhip_pipe** pp, const char* who, const TunerBankDesc* b, int block_size_out, int input_type, int max_type,
                         PipeKind kind, BankForm::Kind form, int nstate)
{
#define BANK_PIPE_REQUIRE(cond, what)                                                     \
    if (!(cond)) {                                                                        \
        set_error("%s" what ": requirement `%s` violated", who, #cond);                   \
        return SDRHIP_ERR_ARG;                                                            \
    }
    BANK_PIPE_REQUIRE(pp != nullptr, "");
    *pp = nullptr;
    BANK_PIPE_REQUIRE(b != nullptr, ": null bank");
    BANK_PIPE_REQUIRE(block_size_out > 0, ": block_size_out > 0");
    if (max_type == 1) BANK_PIPE_REQUIRE(input_type == 0 || input_type == 1, ": input_u8 is 0 (cfloat blocks) or 1 (u8 IQ blocks)");
    BANK_PIPE_REQUIRE(input_type >= 0 && input_type <= 2, ": input_type is 0 (cfloat blocks), 1 (u8 IQ) or 2 (int16 IQ)");
#undef BANK_PIPE_REQUIRE
    const FirDesc* f = &b->ch[0]->fir;
    const int K = (int)b->ch.size();
    int rc = pipe_new(pp, kind, f, nullptr, block_size_out, true, form == BankForm::IQ, 1, f->factor, f->Lp, (InFmt)input_type);
    if (rc != SDRHIP_OK) return rc;
    sdrhip_pipe* p = *pp;
    p->bank = b;
    p->form = form;
    p->pol = {/* stream0 */ nstate > 0, /* in_place */ K == 1 && form == BankForm::IQ, /* align_first */ true, /* iq_always */ form == BankForm::ENV};
    p->am_dc = form == BankForm::ENV && nstate == 1;
    if (K > 1) p->eng.set_rows(K);
    ChannelState& st = nstate == 2 ? p->fm : p->dc;
    st.pingpong = nstate == 2;
    for (int i = 0; i < nstate && rc == SDRHIP_OK; i++) rc = pipe_dev_state(pp, st.buf[i], (size_t)K * 2 * sizeof(float), nullptr, who);
    return rc;
}

int sdrhip_pipe_tuner_bank(sdrhip_pipe** pp, const sdrhip_tuner_bank* b, int block_size_out, int input_u8)
{
    return bank_pipe_new(pp, "sdrhip_pipe_tuner_bank", b, block_size_out, input_u8, 1, PK_TUNER_BANK, BankForm::IQ, 0);
}

int sdrhip_pipe_tuner_bank_i16(sdrhip_pipe** pp, const sdrhip_tuner_bank* b, int block_size_out)
{
    return bank_pipe_new(pp, "sdrhip_pipe_tuner_bank_i16", b, block_size_out, IN_I16, 2, PK_TUNER_BANK, BankForm::IQ, 0);
}

int sdrhip_pipe_am_bank(sdrhip_pipe** pp, const sdrhip_am_bank* a, int block_size_out, int input_type)
{
    return bank_pipe_new(pp, "sdrhip_pipe_am_bank", a ? a->tb : nullptr, block_size_out, input_type, 2, PK_AM_BANK, BankForm::ENV,
                         a && a->dc_block != 0 ? 1 : 0);
}

int sdrhip_pipe_nfm_bank(sdrhip_pipe** pp, const sdrhip_nfm_bank* a, int block_size_out, int input_type)
{
    return bank_pipe_new(pp, "sdrhip_pipe_nfm_bank", a ? a->tb : nullptr, block_size_out, input_type, 2, PK_NFM_BANK, BankForm::PHASE, 2);
}

// The audio Pipes: the bank's Pipe with block_size_out = the tail's block, >-> firResampler(block) >-> firFilter(block) >-> (* gain),
// the tail on the device rows (rows_tail, pipes_fir.cpp).  The tail is borrowed, as the bank is.
static int bank_audio_pipe_new(sdrhip_pipe** pp, const char* who, const TunerBankDesc* b, const sdrhip_audio_tail* tail, int input_type,
                               PipeKind kind, BankForm::Kind form, int nstate)
{
    if (pp != nullptr) *pp = nullptr;
    const int64_t block = sdrhip_audio_tail_block(tail);
    if (pp == nullptr || tail == nullptr || block < 1 || block > (int64_t)0x7fffffff) {
        set_error("%s: requirement `a pipe pointer, an audio tail, and a tail created with a block of at least 1` violated", who);
        return SDRHIP_ERR_ARG;
    }
    int rc = bank_pipe_new(pp, who, b, (int)block, input_type, 2, kind, form, nstate);
    if (rc != SDRHIP_OK) return rc;
    (*pp)->tail = tail;
    (*pp)->pol.stream0 = true;                 // (the bank part's rows live on the device from submission to submission)
    return SDRHIP_OK;
}

int sdrhip_pipe_am_bank_audio(sdrhip_pipe** pp, const sdrhip_am_bank* a, const sdrhip_audio_tail* tail, int input_type)
{
    return bank_audio_pipe_new(pp, "sdrhip_pipe_am_bank_audio", a ? a->tb : nullptr, tail, input_type, PK_AM_BANK_AUDIO, BankForm::ENV,
                               a && a->dc_block != 0 ? 1 : 0);
}

int sdrhip_pipe_nfm_bank_audio(sdrhip_pipe** pp, const sdrhip_nfm_bank* a, const sdrhip_audio_tail* tail, int input_type)
{
    return bank_audio_pipe_new(pp, "sdrhip_pipe_nfm_bank_audio", a ? a->tb : nullptr, tail, input_type, PK_NFM_BANK_AUDIO, BankForm::PHASE, 2);
}

// The narrow bank's Pipe: firDecimator deci1 block_mid >-> firDecimator deci2 block_size_out >-> P.map (magnitude | fmDemod)
// [>-> dcBlockingFilter] for the K channels.  The narrow bank (and through it the tuner bank and the second decimator) is borrowed.
int sdrhip_pipe_narrow_bank(sdrhip_pipe** pp, const sdrhip_narrow_bank* nb, int block_mid, int block_size_out, int input_type)
{
    const char* who = "sdrhip_pipe_narrow_bank";
    if (pp != nullptr) *pp = nullptr;
    if (pp == nullptr || nb == nullptr) {
        set_error("%s: requirement `a pipe pointer and a narrow bank` violated", who);
        return SDRHIP_ERR_ARG;
    }
    // after a crossover the rest of a block of block_mid still holds one whole second filter (the reference's `assert "decimate 1"`)
    if (block_mid < nb->d2->Lp + nb->d2->factor) {
        set_error("%s: requirement `block_mid >= numCoeffs + factor of the second decimator` violated", who);
        return SDRHIP_ERR_ARG;
    }
    const int nstate = nb->form == NARROW_FM ? 2 : nb->dc_block ? 1 : 0;       // fmDemod's pairs, or dcBlocker's behind the envelope
    int rc = bank_pipe_new(pp, who, nb->tb, block_size_out, input_type, 2, PK_NARROW_BANK, BankForm::IQ, nstate);
    if (rc != SDRHIP_OK) return rc;
    sdrhip_pipe* p = *pp;
    p->narrow = nb;
    p->block_mid = block_mid;
    p->cplx_out = false;                       // the chunk and the fifo hold one float per stage-2 output
    p->y.width = 2;                            // ... the carried stage-1 outputs are complex
    p->pol.stream0 = true;
    return SDRHIP_OK;
}

// The narrow bank's Pipe with the audio tail behind it on the device: ... >-> firResampler(block) >-> firFilter(block) >-> (* gain), block
// = the tail's block, which is the second decimator's output block too.  The kind stays PK_NARROW_BANK: it is a narrow-bank pipe with
// `tail` set as well as `narrow` (the second rows carry, pipe.hpp).  Every refusal comes before any device work.
int sdrhip_pipe_narrow_bank_audio(sdrhip_pipe** pp, const sdrhip_narrow_bank* nb, const sdrhip_audio_tail* tail, int block_mid, int input_type)
{
    const char* who = "sdrhip_pipe_narrow_bank_audio";
    if (pp != nullptr) *pp = nullptr;
    const int64_t block = sdrhip_audio_tail_block(tail);
    if (pp == nullptr || nb == nullptr || tail == nullptr || block < 1 || block > (int64_t)0x7fffffff) {
        set_error("%s: requirement `a pipe pointer, a narrow bank, an audio tail, and a tail created with a block of at least 1` violated", who);
        return SDRHIP_ERR_ARG;
    }
    int rc = sdrhip_pipe_narrow_bank(pp, nb, block_mid, (int)block, input_type);
    if (rc != SDRHIP_OK) {
        if (rc == SDRHIP_ERR_ARG)
            set_error("%s: refused as sdrhip_pipe_narrow_bank refuses it: block_mid >= numCoeffs + factor of the second decimator, input_type 0 .. 2", who);
        return rc;
    }
    (*pp)->tail = tail;
    return SDRHIP_OK;
}

int sdrhip_pipe_rows(const sdrhip_pipe* p)
{
    SDRHIP_REQUIRE(p != nullptr, "sdrhip_pipe_rows");
    return p->rows();
}

int sdrhip_pipe_fir_resampler(sdrhip_pipe** pp, const sdrhip_resampler* r, int block_size_out)
{
    SDRHIP_REQUIRE(pp && r && block_size_out > 0, "sdrhip_pipe_fir_resampler");
    SDRHIP_REQUIRE(r->Lp >= r->D, "sdrhip_pipe_fir_resampler: padded filter shorter than the decimation step: the reference Pipe "
                                  "mis-steps at buffer boundaries (Filter.hs:702-709)");
    return pipe_new(pp, PK_RESAMPLER, nullptr, r, block_size_out, r->cplx, r->cplx, r->I, r->D, r->Lp);
}

int sdrhip_pipe_fm_demod(sdrhip_pipe** pp)
{
    SDRHIP_REQUIRE(pp != nullptr, "sdrhip_pipe_fm_demod");
    return pipe_new(pp, PK_DEMOD, nullptr, nullptr, 0, true, false, 1, 1, 1);
}

int sdrhip_pipe_am_demod(sdrhip_pipe** pp)
{
    SDRHIP_REQUIRE(pp != nullptr, "sdrhip_pipe_am_demod");
    return pipe_new(pp, PK_AM, nullptr, nullptr, 0, true, false, 1, 1, 1);
}

int sdrhip_pipe_dc_blocker(sdrhip_pipe** pp)
{
    SDRHIP_REQUIRE(pp != nullptr, "sdrhip_pipe_dc_blocker");
    int rc = pipe_new(pp, PK_DCBLOCK, nullptr, nullptr, 0, false, false, 1, 1, 1);
    if (rc != SDRHIP_OK) return rc;
    return pipe_dev_state(pp, (*pp)->map_state, 16, nullptr, "sdrhip_pipe_dc_blocker");       // func 0 0, Filter.hs:732
}

int sdrhip_pipe_agc(sdrhip_pipe** pp, float mu, float reference)
{
    SDRHIP_REQUIRE(pp != nullptr, "sdrhip_pipe_agc");
    int rc = pipe_new(pp, PK_AGC, nullptr, nullptr, 0, true, true, 1, 1, 1);
    if (rc != SDRHIP_OK) return rc;
    (*pp)->agc_mu = mu;
    (*pp)->agc_ref = reference;
    const float init[4] = {1.0f, 0.0f, 0.0f, 0.0f};                           // pMapAccum (agc mu reference) 1, Util.hs:348
    return pipe_dev_state(pp, (*pp)->map_state, sizeof init, init, "sdrhip_pipe_agc");
}

// De-emphasis: a second form of the one-pole map kind (PK_DCBLOCK with deemph_alpha set), as sdrhip_pipe_narrow_bank_audio is a form of
// kind 14.  The state on the device is {y, 0, alpha, 0}: the kernels read and write the first float only, and alpha in the third is what
// tells a saved state from a dcBlocker's (whose third float is 0) and from one of another alpha (pipes_state.cpp).
int sdrhip_pipe_deemph(sdrhip_pipe** pp, float alpha)
{
    if (pp != nullptr) *pp = nullptr;
    SDRHIP_REQUIRE(pp != nullptr && alpha > 0.0f && alpha <= 1.0f, "sdrhip_pipe_deemph: a pipe pointer and 0 < alpha <= 1");
    int rc = pipe_new(pp, PK_DCBLOCK, nullptr, nullptr, 0, false, false, 1, 1, 1);
    if (rc != SDRHIP_OK) return rc;
    (*pp)->deemph_alpha = alpha;
    const float init[4] = {0.0f, 0.0f, alpha, 0.0f};
    return pipe_dev_state(pp, (*pp)->map_state, sizeof init, init, "sdrhip_pipe_deemph");
}

// ---- map stages (fmDemod, amDemod, dcBlockingFilter, agcPipe, de-emphasis): one output vector per input vector ---------------------
// Blocks are staged one behind the other in the slot's pinned buffer and go out as ONE run over all of them -- the carry of a
// block is its predecessor's last sample (fmDemod, Demod.hs:41,46) / the filter's running pair kept on the device
// (dcBlockingFilter, Filter.hs:730-739), which is exactly what a run over the concatenation computes (amDemod carries nothing); the block lengths are
// remembered for the pops.  Submission is adaptive as for the FIR-like stages.  Runs of up to kDirectBytes read and write
// pinned memory in place; larger ones go through the copy engines.  Both launch on the first compute stream.
static int map_submit(sdrhip_pipe* p)
{
    HostStream& e = p->eng;
    const int n = e.staged;
    if (n == 0) return SDRHIP_OK;
    const size_t ein = (size_t)p->esz_in() * 4;
    // (dcBlockingFilter and agcPipe never in place: their lanes re-read their run-in and a short block is one lane's dependent
    // loads)
    const bool direct = p->direct_ok && (p->kind == PK_DEMOD || p->kind == PK_AM) && (size_t)n * ein <= sdrhip_pipe::kDirectBytes;
    const float* h = (const float*)e.staged_base();
    return e.submit(direct ? HostStream::kInPlace : HostStream::kCopyEngines, e.compute[0], h, (size_t)n * ein,
                    (int64_t)n * p->esz_out(), [&](hipStream_t s, const void* d_in, void* d_out) {
        if (p->kind == PK_DEMOD) {
            launch_fm_demod_fast(s, (const float*)d_in, (float*)d_out, n, false, p->last_re, p->last_im);
            p->last_re = h[2 * (size_t)(n - 1)];
            p->last_im = h[2 * (size_t)(n - 1) + 1];
        } else if (p->kind == PK_AM) {
            launch_am_demod_rows(s, 1, (const float*)d_in, 0, (float*)d_out, 0, n);
        } else if (p->kind == PK_AGC) {
            int rc = grow(p->map_ws, agc_workspace_bytes(n), s);
            if (rc != SDRHIP_OK) return rc;
            launch_agc(s, n, p->agc_mu, p->agc_ref, 1.0f, (const float*)d_in, (float*)d_out, (float*)p->map_state.p, p->map_ws.p, 0,
                       (const float*)p->map_state.p);
        } else if (p->deemph_alpha != 0.0f) {
            // the auto rule with a workspace, whatever route a test has forced: a forced route need not fit a submission
            int rc = grow(p->map_ws, deemph_rows_workspace_bytes(1, n), s);
            if (rc != SDRHIP_OK) return rc;
            DeemphPlan plan;
            (void)deemph_plan(1, n, p->deemph_alpha, 0, true, DEEMPH_AUTO, &plan);
            launch_deemph_rows(s, plan, 1, n, p->deemph_alpha, 0.0f, (const float*)p->map_state.p, (const float*)d_in, n, (float*)d_out, n,
                               (float*)p->map_state.p, p->map_ws.p);
        } else {
            int rc = grow(p->map_ws, dc_blocker_workspace_bytes(n), s);
            if (rc != SDRHIP_OK) return rc;
            launch_dc_blocker(s, n, 0.0f, 0.0f, (const float*)d_in, (float*)d_out, (float*)p->map_state.p, p->map_ws.p, 0,
                              (const float*)p->map_state.p);
        }
        SDRHIP_CHECK_HIP(hipGetLastError());
        return SDRHIP_OK;
    });
}

static int map_push(sdrhip_pipe* p, const float* block, int n)
{
    HostStream& e = p->eng;
    int rc;
    const size_t ein = (size_t)p->esz_in() * 4;
    const int64_t cap_bytes = p->adaptive > 1 ? sdrhip_pipe::adaptive_bytes() : 0;   // what may pile up before a push has to go out
    // room for this block behind what is staged: a pinned buffer does not grow with staged blocks in it
    if (e.staged > 0 && ((size_t)(e.staged + n) * ein > e.slot[e.cur()].hin.cap || (int64_t)e.staged + n > (1 << 30)) &&
        (rc = map_submit(p)) != SDRHIP_OK) return rc;
    if (e.staged == 0) {
        // the slot's previous submission harvested, and room for what may pile up, sized by the blocks this pipe actually sees
        // (not the whole cap for tiny blocks)
        const int64_t pile = p->adaptive > 1 ? (int64_t)p->adaptive * (int64_t)n * (int64_t)ein : 0;
        const size_t want_cap = (size_t)(pile < cap_bytes ? pile : cap_bytes);
        if ((rc = e.open_slot((size_t)n * ein > want_cap ? (size_t)n * ein : want_cap, 0)) != SDRHIP_OK) return rc;
    }
    memcpy(e.write_pos(), block, (size_t)n * ein);
    e.staged += n;
    p->demod_blocks.push_back(n);
    const int64_t pushes_before = e.pushes;
    const bool room = (int64_t)(e.staged + n) * (int64_t)ein <= cap_bytes && (size_t)(e.staged + n) * ein <= e.slot[e.cur()].hin.cap;
    if (!room || !e.next_in_flight()) {
        if ((rc = map_submit(p)) != SDRHIP_OK) return rc;
    }
    if (e.pushes != pushes_before && (rc = e.harvest_done()) != SDRHIP_OK) return rc;
    return ready_blocks(p);
}

int sdrhip_pipe_push(sdrhip_pipe* p, const float* block, int n)
{
    SDRHIP_REQUIRE(p != nullptr && block != nullptr && n > 0, "sdrhip_pipe_push");
    SDRHIP_REQUIRE(p->fmt == IN_CF32, p->fmt == IN_U8 ? "sdrhip_pipe_push: this pipe takes u8 IQ blocks (sdrhip_pipe_push_u8)"
                                                       : "sdrhip_pipe_push: this pipe takes int16 IQ blocks (sdrhip_pipe_push_i16)");
    if (p->kind == PK_SPECTRUM) return spectrum_push(p, block, n);
    return p->is_map() ? map_push(p, block, n) : fir_like_push(p, block, n);
}

int sdrhip_pipe_push_u8(sdrhip_pipe* p, const uint8_t* iq, int n_samples)
{
    SDRHIP_REQUIRE(p != nullptr && iq != nullptr && n_samples > 0, "sdrhip_pipe_push_u8");
    SDRHIP_REQUIRE(p->fmt == IN_U8, p->fmt == IN_I16 ? "sdrhip_pipe_push_u8: this pipe takes int16 IQ blocks (sdrhip_pipe_push_i16)"
                                                     : "sdrhip_pipe_push_u8: this pipe takes float blocks (sdrhip_pipe_push)");
    return p->kind == PK_SPECTRUM ? spectrum_push(p, iq, n_samples) : fir_like_push(p, iq, n_samples);
}

int sdrhip_pipe_push_i16(sdrhip_pipe* p, const int16_t* iq, int n_samples)
{
    SDRHIP_REQUIRE(p != nullptr && iq != nullptr && n_samples > 0, "sdrhip_pipe_push_i16");
    SDRHIP_REQUIRE(p->fmt == IN_I16, p->fmt == IN_U8 ? "sdrhip_pipe_push_i16: this pipe takes u8 IQ blocks (sdrhip_pipe_push_u8)"
                                                     : "sdrhip_pipe_push_i16: this pipe takes float blocks (sdrhip_pipe_push)");
    return p->kind == PK_SPECTRUM ? spectrum_push(p, iq, n_samples) : fir_like_push(p, iq, n_samples);
}

int sdrhip_pipe_set_coalesce(sdrhip_pipe* p, int blocks)
{
    SDRHIP_REQUIRE(p != nullptr && blocks >= 0, "sdrhip_pipe_set_coalesce");
    SDRHIP_REQUIRE(!p->is_map(), "sdrhip_pipe_set_coalesce: filter / decimator / resampler pipes only");
    SDRHIP_REQUIRE(p->eng.staged == 0, "sdrhip_pipe_set_coalesce: blocks are staged (flush first)");
    SDRHIP_REQUIRE(blocks <= 1 || p->uniform_n == 0 || (int64_t)blocks * p->uniform_n <= (int64_t)1 << 30,
                   "sdrhip_pipe_set_coalesce: coalesced batch too large");
    p->coalesce = blocks;
    return SDRHIP_OK;
}

int sdrhip_pipe_set_adaptive(sdrhip_pipe* p, int max_blocks)
{
    SDRHIP_REQUIRE(p != nullptr && max_blocks >= 0 && max_blocks != 1, "sdrhip_pipe_set_adaptive: 0 (off) or at least two blocks");
    SDRHIP_REQUIRE(p->eng.staged == 0, "sdrhip_pipe_set_adaptive: blocks are staged (flush first)");
    p->adaptive = max_blocks;
    return SDRHIP_OK;
}

// the staging memory of the next push, for the three input types (`who` names the caller in a refusal)
static void* pipe_input_buffer(sdrhip_pipe* p, int n, InFmt fmt, const char* who)
{
    if (p == nullptr || n <= 0 || p->is_map()) { set_error("%s: filter / decimator / resampler pipes, n > 0", who); return nullptr; }
    if (p->fmt != fmt) {
        set_error("%s: this pipe takes %s", who, p->fmt == IN_U8 ? "u8 IQ blocks (sdrhip_pipe_input_buffer_u8)"
                                               : p->fmt == IN_I16 ? "int16 IQ blocks (sdrhip_pipe_input_buffer_i16)"
                                                                  : "float blocks (sdrhip_pipe_input_buffer)");
        return nullptr;
    }
    HostStream& e = p->eng;
    if (p->kind == PK_SPECTRUM) {
        // behind what is staged (rows waiting for a coalesce count or a busy GPU); a push that completes no row copies it to the tail
        if ((int64_t)e.staged + n > (int64_t)1 << 30) { set_error("%s: too many samples staged", who); return nullptr; }
        p->lent = 0;
        if (spectrum_open_slot(p, (int64_t)e.staged + n) != SDRHIP_OK) return nullptr;
        p->lent = n;
        return e.write_pos();
    }
    const int ce = p->coalesce_eff(p->uniform_n ? p->uniform_n : n);
    const bool coalescing = ce > 1 && p->all_uniform && (p->uniform_n == 0 || p->uniform_n == n);
    if (!coalescing && e.staged > 0 && fir_submit(p, e.staged, p->uniform_n) != SDRHIP_OK) return nullptr;
    // a fresh pipe has no uniform size yet: the block about to be pushed defines it, so size the buffer for a whole
    // coalesced batch of such blocks now (growing it at the push would move the block the caller is about to fill)
    const int64_t cap = coalescing ? (int64_t)ce * (p->uniform_n ? p->uniform_n : n) : n;
    if (cap > (int64_t)1 << 30) { set_error("%s: coalesced batch too large", who); return nullptr; }
    if (p->open_slot((size_t)(cap > e.staged + n ? cap : e.staged + n)) != SDRHIP_OK) return nullptr;
    p->lent = n;
    return e.write_pos();
}

float* sdrhip_pipe_input_buffer(sdrhip_pipe* p, int n) { return (float*)pipe_input_buffer(p, n, IN_CF32, "sdrhip_pipe_input_buffer"); }

uint8_t* sdrhip_pipe_input_buffer_u8(sdrhip_pipe* p, int n_samples)
{
    return (uint8_t*)pipe_input_buffer(p, n_samples, IN_U8, "sdrhip_pipe_input_buffer_u8");
}

int16_t* sdrhip_pipe_input_buffer_i16(sdrhip_pipe* p, int n_samples)
{
    return (int16_t*)pipe_input_buffer(p, n_samples, IN_I16, "sdrhip_pipe_input_buffer_i16");
}

int sdrhip_pipe_poll(sdrhip_pipe* p)
{
    SDRHIP_REQUIRE(p != nullptr, "sdrhip_pipe_poll");
    int rc = p->eng.harvest_done();
    if (rc != SDRHIP_OK) return rc;
    return ready_blocks(p);
}

int sdrhip_pipe_flush(sdrhip_pipe* p)
{
    SDRHIP_REQUIRE(p != nullptr, "sdrhip_pipe_flush");
    int rc;
    if (p->kind == PK_SPECTRUM) {
        if ((rc = spectrum_settle(p)) != SDRHIP_OK) return rc;
    } else if (p->eng.staged > 0 && (rc = p->is_map() ? map_submit(p) : fir_submit(p, p->eng.staged, p->uniform_n)) != SDRHIP_OK) return rc;
    if ((rc = p->eng.flush()) != SDRHIP_OK) return rc;
    return ready_blocks(p);
}

int sdrhip_pipe_pop(sdrhip_pipe* p, float* out, int capacity)
{
    SDRHIP_REQUIRE(p != nullptr && out != nullptr, "sdrhip_pipe_pop");
    SDRHIP_REQUIRE(p->rows() == 1, "sdrhip_pipe_pop: a pipe of more than one row pops all of them at once (sdrhip_pipe_pop_rows)");
    if (ready_blocks(p) <= 0) return 0;
    int len = p->is_map() ? p->demod_blocks.front() : p->block_out;
    SDRHIP_REQUIRE(capacity >= len, "sdrhip_pipe_pop: capacity smaller than the block");
    p->eng.take((size_t)len * p->esz_out(), out);
    if (p->is_map()) p->demod_blocks.pop_front();
    return len;
}

int sdrhip_pipe_pop_rows(sdrhip_pipe* p, float* out, int64_t row_stride, int max_blocks)
{
    SDRHIP_REQUIRE(p != nullptr && out != nullptr && max_blocks >= 0, "sdrhip_pipe_pop_rows");
    SDRHIP_REQUIRE(!p->is_map(), "sdrhip_pipe_pop_rows: filter / decimator / resampler / tuner pipes (blocks of block_size_out)");
    const int64_t block_floats = (int64_t)p->block_out * p->esz_out();
    SDRHIP_REQUIRE(row_stride >= (int64_t)max_blocks * block_floats, "sdrhip_pipe_pop_rows: a row holds max_blocks blocks");
    const int ready = ready_blocks(p);
    const int nb = ready < max_blocks ? ready : max_blocks;
    if (nb > 0) p->eng.take_rows((size_t)nb * (size_t)block_floats, out, row_stride);
    return nb;
}

void sdrhip_pipe_destroy(sdrhip_pipe* p)
{
    // the borrowed spectrum object outlives the pipe's streams: it must not remember one of them as its scratch's last user
    if (p != nullptr && p->kind == PK_SPECTRUM)
        for (hipStream_t st : p->eng.compute)
            if (st) spectrum_forget_stream(p->sp.spec, st);
    delete p;
}

}  // extern "C"
