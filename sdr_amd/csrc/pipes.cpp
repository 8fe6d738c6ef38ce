// pipes.cpp -- layer (3): the reference's Pipes operators on HOST blocks.
//
//   firFilter    Filter.hs:532-569      firDecimator  Filter.hs:574-611
//   firResampler Filter.hs:679-727      fmDemod       Demod.hs:40-46
//   amDemod      P.map (VG.map magnitude), the Readme's AM receiver
//
// The reference's state machines alternate `simple` (outputs whose window fits in
// the current input buffer: the C SIMD kernel) and `crossover` (outputs straddling
// two buffers: the sequential Haskell kernel), re-blocking the outputs into vectors
// of exactly blockSizeOut (advanceOutBuf, Filter.hs:516-523: a block is yielded only
// when exactly full).  Here each pushed block triggers at most two launches on the
// pipe's stream -- the Cross outputs straddling the boundary with the previous
// block, then the One outputs inside the new block -- over a device buffer that
// holds [carried tail | new block].  Block sizes may vary from push to push.
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
// The waterfall Pipe (sdrhip_pipe_spectrum) is the spectrum operator's reducing form on the same engine: blocks of any size in, rows of
// n floats out, the carried tail being the samples from the first row not yet produced onward (spectrum_push / spectrum_submit below).
#include <stdlib.h>
#include <string.h>

#include <deque>

#include "am.hpp"
#include "descriptors.hpp"
#include "host_stream.hpp"
#include "spectrum.hpp"

using namespace sdrhip;

enum PipeKind : int { PK_FILTER, PK_DECIMATOR, PK_RESAMPLER, PK_DEMOD, PK_DCBLOCK, PK_AGC, PK_TUNER, PK_TUNER_BANK, PK_AM, PK_AM_BANK };   // saved states hold the number: new kinds go at the end
// The waterfall Pipe's kind, the next number (10).  It stands behind the list, not in it: tests/test_pipe_am_bank_abi.py pins the line
// above as the ten kinds whose saved states exist in the field.
constexpr PipeKind PK_SPECTRUM = static_cast<PipeKind>(PK_AM_BANK + 1);
// The narrow-band FM bank's Pipe, the next number again (11), behind the list for the same reason.
constexpr PipeKind PK_NFM_BANK = static_cast<PipeKind>(PK_SPECTRUM + 1);
// The audio Pipes of the two banks (sdrhip_pipe_am_bank_audio, sdrhip_pipe_nfm_bank_audio), the next two numbers (12, 13).
constexpr PipeKind PK_AM_BANK_AUDIO = static_cast<PipeKind>(PK_NFM_BANK + 1);
constexpr PipeKind PK_NFM_BANK_AUDIO = static_cast<PipeKind>(PK_NFM_BANK + 2);
// The narrow-channel bank's Pipe (sdrhip_pipe_narrow_bank), the next number (14).
constexpr PipeKind PK_NARROW_BANK = static_cast<PipeKind>(PK_NFM_BANK + 3);

struct sdrhip_pipe {
    PipeKind kind;
    const FirDesc* fir = nullptr;
    const ResampDesc* rs = nullptr;
    const TunerDesc* tuner = nullptr;  // PK_TUNER: the decimator behind the oscillator mix (fir = &tuner->fir)
    // PK_TUNER_BANK: every channel of the bank in lockstep, one output row per channel (the engine's rows); fir = channel 0's decimator,
    // which is every channel's.  fmt: the blocks are cfloat, interleaved u8 IQ (2 bytes per element) or interleaved int16 IQ (4 bytes
    // per element), and stay in that type up to the kernels' loaders
    const TunerBankDesc* bank = nullptr;
    InFmt fmt = IN_CF32;
    // the bank Pipes' output form (descriptors.hpp) and its scratch policy: complex rows in am_iq for EVERY submission, or only for
    // those whose tile part the fused launch does not take (the IQ form has no composed step and no scratch)
    BankForm::Kind form = BankForm::IQ;
    bool iq_always = false;
    // PK_AM_BANK: the AM bank's Pipe -- the tuner bank's Pipe with ONE float per output (the envelope; bank = the AM bank's tuner bank)
    // and, with am_dc, dcBlocker behind it on the device: its K state pairs live in dc_state, the envelope rows and dcBlocker's
    // workspace in dc_ws, and EVERY submission goes to compute stream 0, so each is ordered behind its predecessor by the stream.
    // am_iq[slot]: complex rows of a submission the fused launch does not serve (another order or factor), one buffer per slot because
    // without am_dc the slots' submissions run on streams of their own.
    bool am_dc = false;
    DevBuf am_iq[HostStream::kMaxSlots];
    // PK_NFM_BANK: the narrow-band FM bank's Pipe -- the tuner bank's Pipe with ONE float per output, fmDemod of each channel over the
    // whole stream.  Every channel's last decimated output lives in device memory: a launch reads nfm_state[nfm_cur] and writes the
    // other array (the two must not overlap: kernels_tuner_bank.hip), and the host swaps them after every launch.  Consecutive
    // submissions depend on each other through that state, so EVERY launch goes to compute stream 0 (as with am_dc).  Submissions the
    // fused launch does not serve go through am_iq.
    DevBuf nfm_state[2];
    int nfm_cur = 0;
    // PK_AM_BANK_AUDIO / PK_NFM_BANK_AUDIO: the bank's Pipe with the audio tail (a BORROWED sdrhip_audio_tail) behind it on the device.
    // The bank part of a submission is the bank Pipe's, but writes its demodulated rows into y_rows[y_cur] (K rows of y_stride floats)
    // behind the y_n elements carried from earlier submissions; row element 0 is demodulated output m_done - y_n of the stream.  One
    // audio_tail run then computes the audio outputs [a_done, ready(m_end)) into the result chunk, and the elements from the next
    // output's first input on are copied to the front of the other buffer (a 2-D device copy on the same stream).  Everything goes to
    // compute stream 0.  block_out is the tail's block.
    const sdrhip_audio_tail* tail = nullptr;
    DevBuf y_rows[2], tail_ws;
    int y_cur = 0;
    int64_t y_stride = 0, y_n = 0, a_done = 0;
    // PK_NARROW_BANK: the tuner bank's Pipe with the narrow bank's stage 2 (a BORROWED sdrhip_narrow_bank: second decimator, demodulator,
    // dcBlocker) behind it on the device, by the audio Pipes' mechanism with COMPLEX elements: the bank part writes complex rows into
    // y_rows[y_cur] behind the y_n carried stage-1 outputs, one narrow_stage2 run with seam_block2 = block_mid computes the stage-2
    // outputs [a_done, narrow_ready(m_end)) into the chunk -- stage 2 sees whole blocks of block_mid only, as the second firDecimator
    // behind `firDecimator deci1 block_mid` does -- and the elements from stage-1 output a_end * D2 on are carried.  fmDemod's pairs
    // live in nfm_state (swapped after every narrow run), dcBlocker's in dc_state.  block_out is the Pipe's own output block.
    const NarrowBankDesc* narrow = nullptr;
    int64_t block_mid = 0;
    bool rows_tail() const { return tail != nullptr || narrow != nullptr; }
    int yw() const { return narrow ? 2 : 1; }             // floats per carried element
    int64_t narrow_ready(int64_t m) const
    {
        const int64_t n1 = m / block_mid * block_mid;
        return n1 >= narrow->d2->Lp ? (n1 - narrow->d2->Lp) / narrow->d2->factor + 1 : 0;
    }
    bool am_kind() const { return kind == PK_AM_BANK || kind == PK_AM_BANK_AUDIO; }
    bool nfm_kind() const { return kind == PK_NFM_BANK || kind == PK_NFM_BANK_AUDIO; }
    // PK_SPECTRUM: the waterfall Pipe over a borrowed spectrum object.  Elements are samples in the object's own type (fmt); output
    // blocks are rows of block_out = n floats.  The engine's history holds exactly the carried tail (the samples from the first row
    // not yet produced onward) while nothing is staged; sp_skip samples of the stream are still to be dropped on arrival (hop > n).
    sdrhip_spectrum* spec = nullptr;
    int64_t sp_hop = 0, sp_pos = 0, sp_rows_done = 0, sp_skip = 0;      // sp_pos: samples pushed so far
    int sp_group = 1, sp_reduce = 0, sp_unit = 0;
    double sp_floor_db = 0.0;
    int block_out = 0;
    bool cplx_in = false, cplx_out = false;
    int I = 1, D = 1, Lp = 1;

    // Four slots = submissions in flight (round 3; SDRHIP_STREAM_SLOTS=2..4).  An in-place push of one host block is one small
    // kernel, ~20 us of latency end to end over PCIe, and the host is done submitting it in ~6: the slots keep the GPU fed.
    bool direct_ok = stream_knobs().direct;
    static constexpr size_t kDirectBytes = 512 << 10;     // [tail | staged] up to this size is read in place over PCIe
    static constexpr size_t kAdaptiveBytes = 4 << 20;     // adaptive submission stages at most this much
    int64_t E_prev = 0;     // global end of the previous block
    int64_t m_done = 0;     // outputs computed so far
    float last_re = 0.0f, last_im = 0.0f;  // fmDemod carry (Demod.hs:41,46)
    // coalescing of equal-sized pushes (FIR-like stages); the elements staged in the current slot are the engine's
    int coalesce = 0;          // blocks per submission (0/1: every push)
    // > 1: submit when the next slot is free, else keep staging up to this many blocks.  On by default (SDRHIP_STREAM_ADAPTIVE=0
    // or sdrhip_pipe_set_adaptive(p, 0) switch it off): a source that is slower than the GPU never notices, a faster one
    // gets the throughput of coalesced pushes at the reference's own block size
    int adaptive = (int)stream_knobs().adaptive.value_or(kAdaptiveBlocks);
    static constexpr int kAdaptiveBlocks = 32;
    // blocks per submission in force for blocks of `uni` elements: the adaptive cap stays inside what is read in place
    // an explicit sdrhip_pipe_set_coalesce(p, N > 1) takes precedence: exactly N blocks per submission, as documented
    bool adaptive_on() const { return adaptive > 1 && coalesce <= 1; }
    int coalesce_eff(int uni) const
    {
        if (adaptive_on() && uni > 0) {
            const int64_t esz = (int64_t)ein();
            // (measured, 8192-sample cfloat blocks into firDecimator: batches of up to 0.5 / 1 / 4 / 16 MiB -> 2.7 / 2.3-3.0 /
            // 3.0-4.9 / 3.7-4.8 G elements/s; batches past kDirectBytes go through the copy engines)
            const int64_t fit = adaptive_bytes() / ((int64_t)uni * esz);
            const int64_t b = adaptive < fit ? adaptive : fit;
            if (b >= 2) return (int)b;
        }
        return coalesce;
    }
    static int64_t adaptive_bytes() { return stream_knobs().adaptive_bytes.value_or((int64_t)kAdaptiveBytes); }
    int uniform_n = 0;         // size of the first block; all_uniform: every block so far had it
    bool all_uniform = true;
    int lent = 0;              // elements behind the staged ones the caller may have filled through sdrhip_pipe_input_buffer

    std::deque<int> demod_blocks;      // fmDemod / amDemod / dcBlockingFilter: output block lengths (one per input block)
    DevBuf dc_state, dc_ws;            // dcBlockingFilter: {lastSample, lastOutput} carried on the device; agcPipe: {state}
    float agc_mu = 0.0f, agc_ref = 0.0f;
    bool is_map() const { return kind == PK_DEMOD || kind == PK_DCBLOCK || kind == PK_AGC || kind == PK_AM; }
    bool has_dev_state() const { return (kind == PK_DCBLOCK || kind == PK_AGC) && dc_state.p; }

    int esz_in() const { return cplx_in ? 2 : 1; }
    size_t ein() const { return fmt == IN_U8 ? 2 : fmt == IN_I16 ? 4 : (size_t)esz_in() * 4; }      // bytes per input element
    // the carried tail starts at a multiple of this many elements: 16 bytes of u8 or int16 input (and the 4 every float pipe always had)
    int64_t tail_align() const { return fmt == IN_U8 ? 8 : 4; }
    int rows() const { return eng.rows; }
    int esz_out() const { return cplx_out ? 2 : 1; }
    int64_t in_offset(int64_t m) const { return ceil_div64(m * (int64_t)D, I); }
    // Elements of esz_in() floats; head room for the carried tail of FIR-like pipes.  Declared last: destroyed first, so its
    // streams are idle before the dcBlocker's buffers are freed.
    HostStream eng;
};

// A pipe of the given kind and geometry, with its engine: FIR-like pipes get head room and history for the carried tail,
// E_prev - in_offset(m_done) < (Lp + D) / I + 1 elements, plus up to 3 of alignment slack (7 of a u8 pipe); map pipes carry nothing.
static int pipe_new(sdrhip_pipe** out, PipeKind kind, const FirDesc* fir, const ResampDesc* rs, int block_out, bool cplx_in,
                    bool cplx_out, int I, int D, int Lp, InFmt fmt = IN_CF32)
{
    sdrhip_pipe* p = new sdrhip_pipe();
    p->kind = kind; p->fir = fir; p->rs = rs; p->block_out = block_out;
    p->cplx_in = cplx_in; p->cplx_out = cplx_out; p->fmt = fmt;
    p->I = I; p->D = D; p->Lp = Lp;
    int64_t head_cap = 0;
    if (!p->is_map()) {
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

static int ready_blocks(const sdrhip_pipe* p)
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

// room for `bytes` in a scratch buffer that launches already on stream s may still use: growing frees the old buffer, so they end first
static int grow(DevBuf& b, size_t bytes, hipStream_t s)
{
    if (bytes > b.cap) SDRHIP_CHECK_HIP(hipStreamSynchronize(s));
    return b.ensure(bytes);
}

// ---- the audio Pipes' device rows ---------------------------------------------------------------------------------------------------
// Room for `need` floats per row in both rows buffers.  Growing (the first submission, or a larger push than any before) waits for the
// launches on s that still use the old buffers and moves the y_n carried elements of every row over.
static int audio_rows_room(sdrhip_pipe* p, int64_t need, hipStream_t s)
{
    const int64_t w = p->yw();
    need *= w;
    if (need <= p->y_stride) return SDRHIP_OK;
    const int K = p->rows();
    const int64_t stride = row_floats(need + need / 4 + 512);
    DevBuf bigger[2];
    int rc;
    for (DevBuf& b : bigger)
        if ((rc = b.ensure((size_t)K * (size_t)stride * sizeof(float))) != SDRHIP_OK) return rc;
    SDRHIP_CHECK_HIP(hipStreamSynchronize(s));
    if (p->y_n > 0)
        SDRHIP_CHECK_HIP(hipMemcpy2D(bigger[0].p, (size_t)stride * sizeof(float), p->y_rows[p->y_cur].p, (size_t)p->y_stride * sizeof(float),
                                     (size_t)(p->y_n * w) * sizeof(float), (size_t)K, hipMemcpyDeviceToDevice));
    for (int i = 0; i < 2; i++) {
        std::swap(p->y_rows[i].p, bigger[i].p);
        std::swap(p->y_rows[i].cap, bigger[i].cap);
    }
    p->y_cur = 0;
    p->y_stride = stride;
    return SDRHIP_OK;
}

// Behind the bank part of a submission that wrote demodulated outputs [m_done, m_done + count) of every row: the audio outputs
// [a_done, a_end) into the chunk by ONE audio_tail run (none when a_end == a_done), then the carry -- the elements from
// first_input(a_end) on go to the front of the other rows buffer.
static int audio_rows_tail(sdrhip_pipe* p, hipStream_t s, float* d_chunk, int64_t m_done, int64_t count, int64_t a_end)
{
    const int K = p->rows();
    const int64_t n_y = p->y_n + count, y_base = m_done - p->y_n;
    if (a_end == p->a_done) {
        p->y_n = n_y;
        return SDRHIP_OK;
    }
    float* y = (float*)p->y_rows[p->y_cur].p;
    const size_t ws = sdrhip_audio_tail_workspace_bytes(p->tail, K, n_y);
    int rc = grow(p->tail_ws, ws, s);
    if (rc != SDRHIP_OK) return rc;
    if ((rc = sdrhip_audio_tail_run_rows(p->tail, s, y, p->y_stride, y_base, n_y, d_chunk, a_end - p->a_done, K, p->a_done, a_end, p->tail_ws.p,
                                         ws)) != SDRHIP_OK)
        return rc;
    int64_t keep = m_done + count - sdrhip_audio_tail_first_input(p->tail, a_end);
    if (keep < 0) keep = 0;
    if (keep > n_y) keep = n_y;
    if (keep > 0)
        SDRHIP_CHECK_HIP(hipMemcpy2DAsync(p->y_rows[p->y_cur ^ 1].p, (size_t)p->y_stride * sizeof(float), y + (n_y - keep),
                                          (size_t)p->y_stride * sizeof(float), (size_t)keep * sizeof(float), (size_t)K,
                                          hipMemcpyDeviceToDevice, s));
    p->y_cur ^= 1;
    p->y_n = keep;
    return SDRHIP_OK;
}

// The narrow Pipe's part behind the bank part of a submission that wrote the complex stage-1 outputs [m_done, m_done + count) of every
// row: the stage-2 outputs [a_done, a_end) into the chunk by ONE narrow_stage2 run (none when a_end == a_done) -- the fused launch
// wherever it fits, whatever the bank's route setting and auto rule (those belong to sdrhip_narrow_bank_run) -- then the carry: the
// elements from stage-1 output a_end * D2 on go to the front of the other rows buffer.
static int narrow_rows_tail(sdrhip_pipe* p, hipStream_t s, float* d_chunk, int64_t m_done, int64_t count, int64_t a_end)
{
    const int K = p->rows();
    const NarrowBankDesc* nb = p->narrow;
    const int64_t n_y = p->y_n + count, y_base = m_done - p->y_n;
    if (a_end == p->a_done) {
        p->y_n = n_y;
        return SDRHIP_OK;
    }
    float* y = (float*)p->y_rows[p->y_cur].p;
    const int64_t n = a_end - p->a_done;
    const bool fused = narrow_stage2_fits(nb, K, y, p->y_stride, y_base, p->a_done, a_end, p->block_mid);
    const size_t ws = narrow_stage2_bytes(nb, K, n, fused);
    int rc = grow(p->tail_ws, ws > 16 ? ws : 16, s);
    if (rc != SDRHIP_OK) return rc;
    const bool fm = nb->form == NARROW_FM;
    if (fused && (rc = nb->d2->ensure_device()) != SDRHIP_OK) return rc;
    rc = narrow_stage2(nb, s, fused, y, p->y_stride, y_base, n_y, d_chunk, n, p->a_done, a_end, p->block_mid,
                       fm ? (const float*)p->nfm_state[p->nfm_cur].p : nullptr, fm ? (float*)p->nfm_state[p->nfm_cur ^ 1].p : nullptr,
                       nb->dc_block ? (float*)p->dc_state.p : nullptr, (float*)p->tail_ws.p, ws);
    if (rc != SDRHIP_OK) return rc;
    if (fm) p->nfm_cur ^= 1;
    int64_t keep = m_done + count - a_end * nb->d2->factor;
    if (keep < 0) keep = 0;
    if (keep > n_y) keep = n_y;
    if (keep > 0)
        SDRHIP_CHECK_HIP(hipMemcpy2DAsync(p->y_rows[p->y_cur ^ 1].p, (size_t)p->y_stride * sizeof(float), y + 2 * (n_y - keep),
                                          (size_t)p->y_stride * sizeof(float), (size_t)(2 * keep) * sizeof(float), (size_t)K,
                                          hipMemcpyDeviceToDevice, s));
    p->y_cur ^= 1;
    p->y_n = keep;
    return SDRHIP_OK;
}

// The launches of one submission (fir_submit below), run(k_begin, k_end, seam_block, outputs in front of k_begin in this submission):
// a uniform run is ONE call over [m_done, m_end) with its seams; a ragged block is the Cross call over [m_done, m_split) (seam -1),
// then the One call over [m_split, m_end) (seam 0).  An empty part is no call.
template <class Run>
static int submit_parts(int64_t m_done, int64_t m_split, int64_t m_end, int64_t uniform_seam, Run run)
{
    const int64_t t0 = uniform_seam > 0 ? m_done : m_split;
    int r;
    if (t0 > m_done && (r = run(m_done, t0, (int64_t)-1, (int64_t)0)) != SDRHIP_OK) return r;
    return m_end > t0 ? run(t0, m_end, uniform_seam, t0 - m_done) : SDRHIP_OK;
}

// Submit the n elements staged in the current slot's pinned buffer.  uniform_seam > 0: they are whole blocks of that size
// and so was everything before them, so the seams of the reference's input buffers are the multiples of uniform_seam and
// ONE stream-API run covers the batch (interior seams included).  uniform_seam == 0: a single block of arbitrary size: the
// outputs straddling the boundary with the previous block first (all Cross), then the ones inside the new block (all One).
static int fir_submit(sdrhip_pipe* p, int n, int64_t uniform_seam)
{
    HostStream& e = p->eng;
    const int si = e.cur();
    const size_t ein = p->ein();
    const int64_t E_prev = p->E_prev, E = E_prev + n;
    // outputs computable once these samples are in: window end <= E*I
    int64_t m_end = (E * p->I >= p->Lp) ? (E * p->I - p->Lp) / p->D + 1 : 0;
    // first output starting at/after the previous boundary: everything before it
    // that is not yet done straddles that boundary (Cross)
    int64_t m_split = ceil_div64(E_prev * p->I, p->D);
    if (m_split < p->m_done) m_split = p->m_done;
    // ... unless the Pipe does not cross over at this boundary at all: the first pending output already has its first
    // input in the new block (`VG.length bufIn' == 0 -> simple next`, Filter.hs:707-709; resamplers only)
    if (E_prev > 0 && !seam_has_crossover(E_prev * p->I, p->I, p->D, p->Lp)) m_split = p->m_done;
    // ... and the last of them, when its first input is already in the new block, only if the output block had room for
    // it (kernels.hpp: late_output_is_one)
    if (m_split > p->m_done && late_output_is_one(m_split - 1, E_prev * p->I, p->I, p->D, p->block_out)) m_split--;
    // staging buffer = [carried tail | staged elements]: the tail starts at the first input any pending output needs,
    // rounded down to a multiple of 4 elements, 8 of a u8 pipe (16-byte aligned device reads wherever the block sizes allow)
    int64_t keep_from = p->in_offset(p->m_done);
    if (keep_from > E_prev) keep_from = E_prev;
    keep_from -= keep_from & (p->tail_align() - 1);
    const int64_t tail = E_prev - keep_from;
    const uint8_t* first = e.carry(keep_from, E_prev, n, "pipe");
    if (first == nullptr) return SDRHIP_ERR_STATE;
    const bool direct = p->direct_ok && (size_t)(tail + n) * ein <= sdrhip_pipe::kDirectBytes;
    // in-place pushes go to their slot's own compute stream: nothing push i+1 computes depends on what push i left on the
    // device (the carried tail comes from the host-side history), so consecutive pushes overlap on the GPU
    hipStream_t cs = direct ? e.compute[si] : e.compute[0];
    const int64_t in_base = keep_from, m_done = p->m_done;
    // More than one row never reads its input in place: with K channels in the grid every channel's workgroups would fetch the same
    // tile over the link (the reason the FM bank's stream gives, chain.cpp).  Up to the direct bound such a submission is ONE copy
    // into device memory on the slot's own stream and the launch behind it.
    const int rows = p->rows();
    // The AM bank's Pipe never reads in place, whatever the row count (a stated choice: the FM bank stream's sweep found no in-place
    // region), and with dcBlocker all its launches share compute stream 0: a submission's dcBlocker starts from the state its
    // predecessor's left on the device
    const bool nfm = p->nfm_kind();
    const bool am = p->am_kind() || nfm;      // (the narrow-band FM bank's Pipe makes the same choice)
    const bool audio = p->rows_tail();        // (the bank part's rows live on the device from submission to submission)
    const int eo = p->narrow ? 2 : p->esz_out();      // floats per output of the bank part (the narrow Pipe's is complex, its chunk is not)
    if (p->am_dc || nfm || audio) cs = e.compute[0];
    const HostStream::Route route = !direct ? HostStream::kCopyEngines : (rows > 1 || am) ? HostStream::kSlotStream : HostStream::kInPlace;
    if ((p->kind == PK_TUNER_BANK || p->kind == PK_NARROW_BANK || am) && route != HostStream::kInPlace) {
        // the copy may land anywhere in the slot's device buffer: put the banked launch's first window on a 16-byte boundary there,
        // which the staging buffer cannot promise once a block had an odd size
        const int64_t k0 = uniform_seam > 0 ? m_done : m_split;
        const size_t off = (size_t)(k0 * p->D - keep_from) * ein;
        e.dev_skew = (16 - off % 16) % 16;
    }
    // the audio Pipes: the chunk holds the audio outputs that became ready, [a_done, a_end) of every row
    int64_t a_end = p->a_done;
    if (audio) {
        a_end = p->narrow ? p->narrow_ready(m_end) : sdrhip_audio_tail_ready(p->tail, m_end);
        if (a_end < p->a_done) a_end = p->a_done;
    }
    const int64_t row_len = audio ? a_end - p->a_done : (m_end - m_done) * p->esz_out();
    int rc = e.submit(route, cs, first, (size_t)(tail + n) * ein, rows * row_len, [&](hipStream_t s, const void* d_in, void* d_out) {
        const float* din = (const float*)d_in;
        float* dout = (float*)d_out;
        if (p->bank == nullptr) {
            // filter / decimator / resampler, or the tuner's mix + decimator: in_base is the absolute stream position of din[0], which
            // is what selects the oscillator phase
            return submit_parts(m_done, m_split, m_end, uniform_seam, [&](int64_t k0, int64_t k1, int64_t seam, int64_t off) {
                float* o = dout + off * p->esz_out();
                if (p->kind == PK_RESAMPLER) return resamp_run(p->rs, s, din, in_base, o, k0, k1, seam, seam > 0 ? p->block_out : 0);
                if (p->kind == PK_TUNER) return tuner_run(p->tuner, s, din, IN_CF32, in_base, o, k0, k1, seam);
                return fir_run(p->fir, s, din, false, in_base, o, k0, k1, seam);
            });
        }
        // The banks: every row [cross | one] in the Pipe's form, row_len apart (dev_skew has aligned the tile part's first window).
        // IQ: the bank's own rule picks the banked launch or channel by channel.  Envelopes and phases, one float per output: the
        // fused launch (set) where it fits, else tuner bank + amDemod / fmDemod rows through the slot's complex scratch.
        const int K = rows;
        const int64_t count = m_end - m_done, np = row_floats(count);
        int r;
        // where the form's rows end up: the result chunk, or (the audio Pipes) the device rows buffer behind the carried history
        float* fin = dout;
        int64_t fin_stride = row_len;
        if (audio) {
            if ((r = audio_rows_room(p, p->y_n + count, s)) != SDRHIP_OK) return r;
            fin = (float*)p->y_rows[p->y_cur].p + p->y_n * p->yw();
            fin_stride = p->y_stride;
        }
        float* out = fin;
        int64_t stride = fin_stride;
        if (p->am_dc) {
            // dcBlocker's row form refuses d_in == d_out: the envelope rows pass through dc_ws, its own workspace behind them
            if ((r = grow(p->dc_ws, (size_t)K * (size_t)np * sizeof(float) + dc_blocker_rows_workspace_bytes(K, count), s)) != SDRHIP_OK) return r;
            out = (float*)p->dc_ws.p;
            stride = np;
        }
        BankForm form{p->form};
        // (the fused launch never touches the complex scratch, and 32 channels of it are K * 2 * np floats: a form that keeps it only
        // where the tile part is not the fused launch asks the predicate that bank_form_run asks)
        const int64_t t0 = uniform_seam > 0 ? m_done : m_split;
        float* iq = nullptr;
        if (p->iq_always || (form.kind != BankForm::IQ && m_end > t0 &&
                             !bank_fused_fits(p->bank, bank_geom(p->fir, in_base, t0, m_end, uniform_seam), d_in, p->fmt, form, nullptr))) {
            if ((r = grow(p->am_iq[si], (size_t)K * 2 * (size_t)np * sizeof(float), s)) != SDRHIP_OK) return r;
            iq = (float*)p->am_iq[si].p;
        }
        r = submit_parts(m_done, m_split, m_end, uniform_seam, [&](int64_t k0, int64_t k1, int64_t seam, int64_t off) {
            float* o = out + off * eo;
            if (form.kind == BankForm::PHASE) {
                // each launch takes the state its predecessor left and leaves the next one's in the other array
                form.d_state = (const float*)p->nfm_state[p->nfm_cur].p;
                form.d_final = (float*)p->nfm_state[p->nfm_cur ^ 1].p;
            }
            int rr;
            if (seam < 0) rr = bank_cross(p->bank, s, d_in, p->fmt, in_base, o, stride, k0, k1, form);
            else if (form.kind == BankForm::IQ) rr = tuner_bank_run(p->bank, s, d_in, p->fmt, in_base, o, stride, k0, k1, seam);
            else rr = bank_form_run(p->bank, s, d_in, p->fmt, in_base, o, stride, k0, k1, seam, form, iq);
            if (rr == SDRHIP_OK && form.kind == BankForm::PHASE) p->nfm_cur ^= 1;
            return rr;
        });
        if (r != SDRHIP_OK) return r;
        if (p->am_dc) {
            launch_dc_blocker_rows(s, K, count, out, np, fin, fin_stride, (const float*)p->dc_state.p, (float*)p->dc_state.p,
                                   out + (size_t)K * (size_t)np, 0);
            SDRHIP_CHECK_HIP(hipGetLastError());
        }
        if (p->narrow) return narrow_rows_tail(p, s, dout, m_done, count, a_end);
        return audio ? audio_rows_tail(p, s, dout, m_done, count, a_end) : SDRHIP_OK;
    }, audio && m_end > m_done);
    if (rc != SDRHIP_OK) return rc;
    p->m_done = m_end;
    p->E_prev = E;
    p->a_done = a_end;
    return SDRHIP_OK;
}

// make the current slot writable with room for `elems` staged elements: growth keeps what is staged and what the caller
// was lent behind it (sdrhip_pipe_input_buffer)
static int fir_open_slot(sdrhip_pipe* p, size_t elems)
{
    const size_t ein = p->ein();
    return p->eng.open_slot(elems * ein, (size_t)(p->eng.staged + p->lent) * ein);
}

// the reference's `assert "filter 1" / "decimate 1" / "resample 1"` for a block of n elements arriving at E_at: after the
// crossover the rest of the new buffer must still hold one whole filter
static int fir_check_block(const sdrhip_pipe* p, int64_t E_at, int64_t m_pending, int n)
{
    const int64_t E = E_at + n;
    const int64_t m_end = (E * p->I >= p->Lp) ? (E * p->I - p->Lp) / p->D + 1 : 0;
    int64_t m_split = ceil_div64(E_at * p->I, p->D);
    if (m_split < m_pending) m_split = m_pending;
    if (m_end <= m_split) {
        set_error("pipe: input block of %d elements is shorter than the filter (numCoeffs %d): the reference asserts "
                  "(Filter.hs:544,586,691)", n, p->Lp);
        return SDRHIP_ERR_ARG;
    }
    return SDRHIP_OK;
}

static int fir_like_push(sdrhip_pipe* p, const void* block, int n)
{
    HostStream& e = p->eng;
    int rc;
    const size_t ein = p->ein();
    // the size of the first ACCEPTED block is the uniform size: a block the checks below refuse must not latch it
    const int uni = p->uniform_n == 0 ? n : p->uniform_n;
    const bool all_uniform = p->all_uniform && n == uni;
    const int ce = p->coalesce_eff(uni);
    const bool coalescing = ce > 1 && all_uniform;
    if ((int64_t)ce * uni > (int64_t)1 << 30) {
        set_error("pipe: %d coalesced blocks of %d elements exceed the staging limit", ce, uni);
        return SDRHIP_ERR_ARG;
    }
    // zero-copy push: `block` is the staging buffer's own write position (sdrhip_pipe_input_buffer); noted before the
    // buffer can be re-allocated below (growth keeps the lent region, so the data is then already in place)
    const bool in_place = e.slot[e.cur()].hin.p != nullptr && block == (const void*)e.write_pos();
    const uint64_t pushes_at_entry = (uint64_t)e.pushes;
    if (!coalescing && e.staged > 0) {
        // a block of another size ends the uniform run: what is staged goes out as one uniform batch first
        if ((rc = fir_submit(p, e.staged, p->uniform_n)) != SDRHIP_OK) return rc;
    }
    // that submission moved on to the other slot: a block the caller wrote into the OLD slot's lent region (still intact:
    // the submitted run ends where the lent region starts) is not in place any more and must be copied like any other
    const bool still_in_place = in_place && (uint64_t)e.pushes == pushes_at_entry;
    // the block must be acceptable to the reference's Pipe where it arrives
    const int64_t m_pending = e.staged > 0 ? ((p->E_prev + e.staged) * p->I >= p->Lp ? ((p->E_prev + e.staged) * p->I - p->Lp) / p->D + 1 : 0)
                                           : p->m_done;
    if ((rc = fir_check_block(p, p->E_prev + e.staged, m_pending, n)) != SDRHIP_OK) return rc;
    p->uniform_n = uni;
    p->all_uniform = all_uniform;
    const int64_t cap = coalescing ? (int64_t)ce * p->uniform_n : n;
    if ((rc = fir_open_slot(p, (size_t)(cap > e.staged + n ? cap : e.staged + n))) != SDRHIP_OK) return rc;
    if (!still_in_place) memcpy(e.write_pos(), block, (size_t)n * ein);   // else: the caller filled the staging buffer in place
    p->lent = 0;
    e.staged += n;
    const int64_t pushes_before = e.pushes;
    if (!coalescing) {
        // equal-sized blocks from the start: the seams are the multiples of that size and one run covers Cross and One
        // outputs alike; otherwise (ragged blocks) the two-part submission
        if ((rc = fir_submit(p, e.staged, p->all_uniform ? p->uniform_n : 0)) != SDRHIP_OK) return rc;
    } else if (e.staged >= (int64_t)ce * p->uniform_n || (p->adaptive_on() && !e.next_in_flight())) {
        // (adaptive: a GPU that keeps up gets every push at once; one still busy with the slot this submission would move on
        // to lets the blocks pile up in the staging buffer and takes them as one launch when it frees up)
        if ((rc = fir_submit(p, e.staged, p->uniform_n)) != SDRHIP_OK) return rc;
    }
    // a push that went out also collects whatever the GPU has finished meanwhile (a source slower than the GPU gets the
    // results of push i at push i + 1 instead of i + nslots - 1); staged pushes skip the query
    if (e.pushes != pushes_before && (rc = e.harvest_done()) != SDRHIP_OK) return rc;
    return ready_blocks(p);
}

// ---- the waterfall Pipe (sdrhip_pipe_spectrum) ------------------------------------------------------------------------------------
// With S the samples pushed so far, output row R exists once (R group + group - 1) hop + n <= |S| and is row R of ONE
// sdrhip_spectrum_reduce_run_device over S.  The host keeps the samples from row sp_rows_done's first one onward: the engine's history
// while no row is complete, [history | staged] in the slot's staging buffer once one is (a submission, or rows piling up behind a
// busy GPU / a coalesce count).  A submission is one reduce run over [tail | staged] with rows_out = every complete row.
static constexpr size_t kSpectrumTailBytes = 4 << 20;     // the engine's adaptive staging cap: the bound of the carried tail

static int64_t spectrum_rows_in(const sdrhip_pipe* p, int64_t avail)
{
    if (avail < p->block_out) return 0;
    return ((avail - p->block_out) / p->sp_hop + 1) / p->sp_group;
}

static int spectrum_submit(sdrhip_pipe* p)
{
    HostStream& e = p->eng;
    const int si = e.cur();
    const size_t ein = p->ein();
    const int64_t tail = e.hist_n, have = tail + e.staged, r = spectrum_rows_in(p, have);
    if (r < 1) return SDRHIP_OK;
    uint8_t* first = e.staged_base() - (size_t)tail * ein;
    if (tail > 0) memcpy(first, e.hist.data(), (size_t)tail * ein);
    // The input is never read in place (hop < n reads every sample n / hop times): up to kDirectBytes one copy on the slot's stream
    // and the launch behind it, beyond that the copy engines.  A run that goes through the object's ONE scratch buffer (the hipFFT
    // route, layers of a group past 32 rows) is ordered behind its predecessor by the engine's first compute stream.
    const bool direct = (size_t)have * ein <= sdrhip_pipe::kDirectBytes;
    const bool scratch = spectrum_reduce_uses_scratch(p->spec, p->sp_group);
    hipStream_t cs = direct && !scratch ? e.compute[si] : e.compute[0];
    const int n = p->block_out;
    int rc = e.submit(direct ? HostStream::kSlotStream : HostStream::kCopyEngines, cs, first, (size_t)have * ein, r * n,
                      [&](hipStream_t s, const void* d_in, void* d_out) {
        return sdrhip_spectrum_reduce_run_device(p->spec, s, d_in, have, p->sp_hop, (int)r, p->sp_group, p->sp_reduce, p->sp_unit, p->sp_floor_db,
                                                 (float*)d_out);
    });
    if (rc != SDRHIP_OK) return rc;
    // the next tail starts at stream sample (rows_done + r) group hop: inside [tail | staged] (still in the slot's staging buffer, which
    // nothing writes before the slot is reopened), or `skip` samples beyond its end
    const int64_t used = r * p->sp_group * p->sp_hop;
    if (used < have) {
        e.hist_n = have - used;
        memcpy(e.hist.data(), first + (size_t)used * ein, (size_t)e.hist_n * ein);
    } else {
        e.hist_n = 0;
        p->sp_skip = used - have;
    }
    p->sp_rows_done += r;
    return SDRHIP_OK;
}

// room for `elems` staged elements in the current slot; growth doubles, so that small pushes piling up do not re-pin every time
static int spectrum_open_slot(sdrhip_pipe* p, int64_t elems)
{
    HostStream& e = p->eng;
    const size_t ein = p->ein(), head = (size_t)e.head_cap * ein, cap = e.slot[e.cur()].hin.cap;
    size_t bytes = (size_t)elems * ein;
    if (cap < head + bytes && cap > head && bytes < 2 * (cap - head)) bytes = 2 * (cap - head);
    return e.open_slot(bytes, (size_t)(e.staged + p->lent) * ein);
}

static int spectrum_push(sdrhip_pipe* p, const void* block, int n)
{
    HostStream& e = p->eng;
    const size_t ein = p->ein();
    int rc;
    if ((int64_t)e.staged + n > (int64_t)1 << 30) {
        set_error("pipe: %d samples behind %d staged ones exceed the staging limit", n, e.staged);
        return SDRHIP_ERR_ARG;
    }
    const bool in_place = e.slot[e.cur()].hin.p != nullptr && block == (const void*)e.write_pos();
    // samples between the last produced row's group and the next one's first sample (hop > n) are dropped on arrival
    const int64_t drop = p->sp_skip < n ? p->sp_skip : n;
    const int m = n - (int)drop;
    p->sp_skip -= drop;
    p->sp_pos += n;
    if (!in_place) p->lent = 0;            // a block lent and not pushed is abandoned: growth below need not keep it
    if (m == 0) {
        p->lent = 0;
        return ready_blocks(p);
    }
    if (e.staged == 0 && spectrum_rows_in(p, e.hist_n + m) < 1) {
        // no row yet: the samples join the carried tail (fewer than (group - 1) hop + n of them: the history's size), nothing is launched
        memcpy(e.hist.data() + (size_t)e.hist_n * ein, (const uint8_t*)block + (size_t)drop * ein, (size_t)m * ein);
        e.hist_n += m;
        p->lent = 0;
        return ready_blocks(p);
    }
    if ((rc = spectrum_open_slot(p, (int64_t)e.staged + (in_place ? n : m))) != SDRHIP_OK) return rc;
    // (growth keeps the lent region, so a block the caller filled in place is at the write position of the new buffer too)
    const uint8_t* src = in_place ? e.write_pos() + (size_t)drop * ein : (const uint8_t*)block + (size_t)drop * ein;
    if (src != e.write_pos()) memmove(e.write_pos(), src, (size_t)m * ein);
    p->lent = 0;
    e.staged += m;
    const int64_t r = spectrum_rows_in(p, e.hist_n + e.staged);
    // every push that completes a row goes out at once; coalesce(N > 1) waits for N rows; adaptive lets rows pile up (up to its row
    // count and byte cap) while the slot the submission would move on to is still running
    bool go = true;
    if (p->coalesce > 1) go = r >= p->coalesce;
    else if (p->adaptive > 1)
        go = r >= p->adaptive || (int64_t)(e.hist_n + e.staged) * (int64_t)ein >= sdrhip_pipe::adaptive_bytes() || !e.next_in_flight();
    const int64_t pushes_before = e.pushes;
    if (go && (rc = spectrum_submit(p)) != SDRHIP_OK) return rc;
    if (e.pushes != pushes_before && (rc = e.harvest_done()) != SDRHIP_OK) return rc;
    return ready_blocks(p);
}

// flush / save: every complete row goes out, and what is left of the staged samples (no whole row) joins the history
static int spectrum_settle(sdrhip_pipe* p)
{
    int rc;
    p->lent = 0;
    if (p->eng.staged > 0 && (rc = spectrum_submit(p)) != SDRHIP_OK) return rc;
    return SDRHIP_OK;
}

extern "C" {

int sdrhip_pipe_spectrum(sdrhip_pipe** pp, sdrhip_spectrum* s, int64_t hop, int group, int reduce, int unit, double floor_db)
{
    // (all of it before pipe_new, whose engine creates streams: a refused create has done no device work)
    SDRHIP_REQUIRE(pp != nullptr, "sdrhip_pipe_spectrum");
    *pp = nullptr;
    SDRHIP_REQUIRE(s != nullptr, "sdrhip_pipe_spectrum: null spectrum object");
    SDRHIP_REQUIRE(hop >= 1 && group >= 1, "sdrhip_pipe_spectrum: hop >= 1, group >= 1");
    SDRHIP_REQUIRE(reduce >= SDRHIP_REDUCE_MEAN_POWER && reduce <= SDRHIP_REDUCE_MAX_MAGNITUDE, "sdrhip_pipe_spectrum: reduce out of range");
    SDRHIP_REQUIRE(unit == SDRHIP_UNIT_LINEAR || unit == SDRHIP_UNIT_DB, "sdrhip_pipe_spectrum: unit out of range");
    SDRHIP_REQUIRE(floor_db == floor_db && floor_db - floor_db == 0.0, "sdrhip_pipe_spectrum: floor_db must be finite");
    const int n = spectrum_size_of(s), format = spectrum_format_of(s);
    const InFmt fmt = format == SDRHIP_IQ_U8 ? IN_U8 : format == SDRHIP_IQ_I16 ? IN_I16 : IN_CF32;
    const int64_t sb = in_fmt_bytes(fmt), cap = (int64_t)kSpectrumTailBytes / sb;
    // the carried tail, ((group - 1) hop + n - 1) samples at most, stays within 4 MiB (without overflow: hop <= cap first)
    SDRHIP_REQUIRE(n - 1 <= cap && (group == 1 || (hop <= cap && (int64_t)(group - 1) <= (cap - (n - 1)) / hop)),
                   "sdrhip_pipe_spectrum: ((group - 1) * hop + n - 1) samples of carried tail exceed 4 MiB");
    const int64_t max_tail = (int64_t)(group - 1) * hop + n - 1;
    sdrhip_pipe* p = new sdrhip_pipe();
    p->kind = PK_SPECTRUM;
    p->spec = s;
    p->block_out = n;
    p->cplx_in = true;
    p->cplx_out = false;
    p->fmt = fmt;
    p->sp_hop = hop; p->sp_group = group; p->sp_reduce = reduce; p->sp_unit = unit; p->sp_floor_db = floor_db;
    int rc = p->eng.init(HostStream::kMaxSlots, p->ein(), max_tail > 0 ? max_tail : 1, "pipe: stream/event creation failed");
    if (rc != SDRHIP_OK) {
        delete p;
        return rc;
    }
    *pp = p;
    return SDRHIP_OK;
}

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

// A pipe's state on the device: `bytes` of `buf` (at least 16), zeros -- set on the first compute stream -- or a copy of `init`.  On
// failure the pipe is destroyed and *pp is null.
static int pipe_dev_state(sdrhip_pipe** pp, DevBuf& buf, size_t bytes, const void* init, const char* who)
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

// The four bank Pipes: the checks (all of them before pipe_new, whose engine creates streams: a refused create has done no device
// work), the pipe with one engine row per channel, and the form's state on the device: `nstate` arrays (dc_state; nfm_state[0 .. 1])
// of one pair of floats per channel, zeroed (dcBlocker: func 0 0, Filter.hs:731; fmDemod: every channel starts from (0, 0),
// Demod.hs:41).  max_type: the last input type the call takes (1: sdrhip_pipe_tuner_bank's input_u8).
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
    p->iq_always = form == BankForm::ENV;      // (whether the fused launch takes a submission is left to the launcher)
    p->am_dc = p->am_kind() && nstate == 1;
    if (K > 1) p->eng.set_rows(K);
    DevBuf* state = p->nfm_kind() ? p->nfm_state : &p->dc_state;
    for (int i = 0; i < nstate && rc == SDRHIP_OK; i++) rc = pipe_dev_state(pp, state[i], (size_t)K * 2 * sizeof(float), nullptr, who);
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
// the tail on the device rows (audio_rows_tail above).  The tail is borrowed, as the bank is.
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
    if (rc == SDRHIP_OK) (*pp)->tail = tail;
    return rc;
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
    int rc = bank_pipe_new(pp, who, nb->tb, block_size_out, input_type, 2, PK_NARROW_BANK, BankForm::IQ, 0);
    if (rc != SDRHIP_OK) return rc;
    sdrhip_pipe* p = *pp;
    p->narrow = nb;
    p->block_mid = block_mid;
    p->cplx_out = false;                       // the chunk and the fifo hold one float per stage-2 output
    const size_t bytes = (size_t)p->rows() * 2 * sizeof(float);
    if (nb->form == NARROW_FM)
        for (int i = 0; i < 2 && rc == SDRHIP_OK; i++) rc = pipe_dev_state(pp, p->nfm_state[i], bytes, nullptr, who);
    else if (nb->dc_block)
        rc = pipe_dev_state(pp, p->dc_state, bytes, nullptr, who);
    return rc;
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
    return pipe_dev_state(pp, (*pp)->dc_state, 16, nullptr, "sdrhip_pipe_dc_blocker");       // func 0 0, Filter.hs:732
}

int sdrhip_pipe_agc(sdrhip_pipe** pp, float mu, float reference)
{
    SDRHIP_REQUIRE(pp != nullptr, "sdrhip_pipe_agc");
    int rc = pipe_new(pp, PK_AGC, nullptr, nullptr, 0, true, true, 1, 1, 1);
    if (rc != SDRHIP_OK) return rc;
    (*pp)->agc_mu = mu;
    (*pp)->agc_ref = reference;
    const float init[4] = {1.0f, 0.0f, 0.0f, 0.0f};                           // pMapAccum (agc mu reference) 1, Util.hs:348
    return pipe_dev_state(pp, (*pp)->dc_state, sizeof init, init, "sdrhip_pipe_agc");
}

// ---- map stages (fmDemod, amDemod, dcBlockingFilter, agcPipe): one output vector per input vector ------------------------------
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
            int rc = grow(p->dc_ws, agc_workspace_bytes(n), s);
            if (rc != SDRHIP_OK) return rc;
            launch_agc(s, n, p->agc_mu, p->agc_ref, 1.0f, (const float*)d_in, (float*)d_out, (float*)p->dc_state.p, p->dc_ws.p, 0,
                       (const float*)p->dc_state.p);
        } else {
            int rc = grow(p->dc_ws, dc_blocker_workspace_bytes(n), s);
            if (rc != SDRHIP_OK) return rc;
            launch_dc_blocker(s, n, 0.0f, 0.0f, (const float*)d_in, (float*)d_out, (float*)p->dc_state.p, p->dc_ws.p, 0,
                              (const float*)p->dc_state.p);
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
    if (fir_open_slot(p, (size_t)(cap > e.staged + n ? cap : e.staged + n)) != SDRHIP_OK) return nullptr;
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

// ---- checkpoint / resume (as sdrhip_fm_stream_save / _restore, chain.cpp) -------------------------------------------
// Between two pushes a Pipe's state is its position (elements consumed, outputs produced), the last head_cap input elements,
// the carried fmDemod sample / dcBlocker pair / agc state, and the output not yet popped: what the reference keeps in the Pipe's closure
// (Filter.hs:536-727: overlap remainder, resampler (group, offset); Demod.hs:41,46; Filter.hs:730-739).
namespace {
struct PipeStateHeader {
    uint32_t magic, version;
    int32_t kind, block_out, I, D, Lp, cplx_in, cplx_out, uniform_n, all_uniform, n_blocks;
    int64_t E_prev, m_done, head_cap, hist_n, pending;       // hist_n: elements; pending: floats in the fifo
    float last_re, last_im, dc[4];
};
constexpr uint32_t kPipeMagic = 0x50504453u;   // "SDPP"
// Version 2: a pipe of more than one row or of u8 / int16 input.  The same header, then this, then the engine's state with the history
// in the input's own type (2 bytes per u8 element, 4 per int16 one) and the fifo row after row; input_u8 is the input type: 0 = cfloat,
// 1 = u8, 2 = int16.  Every other pipe writes version 1, byte for byte as before.
struct PipeStateRows {
    int32_t rows, input_u8;
};
static uint32_t pipe_state_version(const sdrhip_pipe* p) { return p->rows() > 1 || p->fmt != IN_CF32 ? 2u : 1u; }
// The AM bank's Pipe appends, behind everything else: dc_block, the number of dcBlocker floats (2 K or 0), and those floats.
struct PipeStateAm {
    int32_t dc_block, n_floats;
};
// The narrow-band FM bank's Pipe appends the same record: dc_block = 0, n_floats = 2 K, and every channel's last decimated (re, im).
struct PipeAmRecord {
    bool present;
    PipeStateAm x;
    void* d_floats;       // where the floats live on the device
    size_t bytes() const { return present ? sizeof x + (size_t)x.n_floats * sizeof(float) : 0; }
};
static PipeAmRecord pipe_state_am(const sdrhip_pipe* p)
{
    if (p->nfm_kind()) return {true, {0, 2 * p->rows()}, p->nfm_state[p->nfm_cur].p};
    if (p->am_kind()) return {true, {p->am_dc ? 1 : 0, p->am_dc ? 2 * p->rows() : 0}, p->dc_state.p};
    return {false, {0, 0}, nullptr};
}
// The audio Pipes append, behind that record: the audio position, the tail's shape (so that a state is restored only into a pipe of
// the same resampler ratio and tap counts) and the y_n carried demodulated elements of every row, row after row.
struct PipeStateAudio {
    int64_t a_done, y_n;
    int32_t shape[4];        // sdrhip_audio_tail_shape: interpolation, decimation, numCoeffsR, numCoeffsF
};
static size_t pipe_state_audio_bytes(const sdrhip_pipe* p)
{
    return p->tail ? sizeof(PipeStateAudio) + (size_t)p->rows() * (size_t)p->y_n * sizeof(float) : 0;
}
// The narrow bank's Pipe appends, behind the (absent) record above: the stage-2 position, what the state may be restored into
// (block_mid, the second decimator's factor and prepared length, the form, dc_block), n_floats state floats (fmDemod's pairs or
// dcBlocker's, 2 K; 0 for the plain envelope) and the y_n carried COMPLEX stage-1 outputs of every row, row after row.
struct PipeStateNarrow {
    int64_t a_done, y_n, block_mid;
    int32_t D2, Lp2, form, dc_block, n_floats, reserved;
};
static PipeStateNarrow pipe_state_narrow(const sdrhip_pipe* p)
{
    const NarrowBankDesc* nb = p->narrow;
    const bool st = nb->form == NARROW_FM || nb->dc_block;
    return {p->a_done, p->y_n, p->block_mid, nb->d2->factor, nb->d2->Lp, nb->form, nb->dc_block, st ? 2 * p->rows() : 0, 0};
}
static void* pipe_narrow_floats(const sdrhip_pipe* p) { return p->narrow->form == NARROW_FM ? p->nfm_state[p->nfm_cur].p : p->dc_state.p; }
static size_t pipe_state_narrow_bytes(const sdrhip_pipe* p)
{
    if (!p->narrow) return 0;
    return sizeof(PipeStateNarrow) + (size_t)pipe_state_narrow(p).n_floats * sizeof(float) + (size_t)p->rows() * (size_t)p->y_n * 2 * sizeof(float);
}
static size_t pipe_state_am_bytes(const sdrhip_pipe* p) { return pipe_state_am(p).bytes() + pipe_state_audio_bytes(p) + pipe_state_narrow_bytes(p); }
static size_t pipe_state_header_bytes(const sdrhip_pipe* p) { return sizeof(PipeStateHeader) + (pipe_state_version(p) == 2 ? sizeof(PipeStateRows) : 0); }
// Version 3: the waterfall Pipe.  This header, the carried tail (tail_n samples in the input's own type), the rows not yet popped
// (pending floats).  pos = samples pushed so far; the tail starts at stream sample rows_done * group * hop = pos - tail_n (skip == 0)
// or lies skip samples beyond pos (tail_n == 0).
struct PipeStateSpectrum {
    uint32_t magic, version;
    int32_t kind, n, input_type, group, reduce, unit;
    int64_t hop;
    double floor_db;
    int64_t pos, rows_done, skip, tail_n, pending;
};
constexpr uint32_t kPipeSpectrumVersion = 3;
}  // namespace

size_t sdrhip_pipe_state_bytes(sdrhip_pipe* p)
{
    if (p == nullptr) return 0;
    // Exact, not an estimate: the pipe is drained here exactly as sdrhip_pipe_save will drain it (what is staged goes out, every
    // slot is harvested into the fifo), so the size returned is what the save that follows needs -- whatever the ratio of
    // the stage and the size of the blocks in flight.  0 = the drain failed (sdrhip_last_error).
    if (sdrhip_pipe_flush(p) < 0) return 0;
    if (p->kind == PK_SPECTRUM) return sizeof(PipeStateSpectrum) + p->eng.state_bytes(p->eng.hist_n, (int64_t)p->eng.pending());
    return pipe_state_header_bytes(p) + p->eng.state_bytes(p->eng.hist_n, (int64_t)p->eng.pending()) + p->demod_blocks.size() * sizeof(int32_t) +
           pipe_state_am_bytes(p);
}

int sdrhip_pipe_save(sdrhip_pipe* p, void* buf, size_t capacity, size_t* used)
{
    SDRHIP_REQUIRE(p != nullptr && buf != nullptr && used != nullptr, "sdrhip_pipe_save");
    int rc = sdrhip_pipe_flush(p);
    if (rc < 0) return rc;
    if (p->kind == PK_SPECTRUM) {
        PipeStateSpectrum x;
        memset(&x, 0, sizeof x);
        x.magic = kPipeMagic;
        x.version = kPipeSpectrumVersion;
        x.kind = (int32_t)p->kind;
        x.n = p->block_out; x.input_type = (int32_t)p->fmt; x.group = p->sp_group; x.reduce = p->sp_reduce; x.unit = p->sp_unit;
        x.hop = p->sp_hop; x.floor_db = p->sp_floor_db;
        x.pos = p->sp_pos; x.rows_done = p->sp_rows_done; x.skip = p->sp_skip; x.tail_n = p->eng.hist_n; x.pending = (int64_t)p->eng.pending();
        const size_t need = sizeof x + p->eng.state_bytes(x.tail_n, x.pending);
        if (capacity < need) {
            set_error("sdrhip_pipe_save: %zu bytes needed, %zu given", need, capacity);
            return SDRHIP_ERR_ARG;
        }
        memcpy(buf, &x, sizeof x);
        (void)p->eng.save((unsigned char*)buf + sizeof x);
        *used = need;
        return SDRHIP_OK;
    }
    PipeStateHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kPipeMagic;
    h.version = pipe_state_version(p);
    h.kind = (int32_t)p->kind;
    h.block_out = p->block_out;
    h.I = p->I; h.D = p->D; h.Lp = p->Lp;
    h.cplx_in = p->cplx_in; h.cplx_out = p->cplx_out;
    h.uniform_n = p->uniform_n; h.all_uniform = p->all_uniform;
    h.n_blocks = (int32_t)p->demod_blocks.size();
    h.E_prev = p->E_prev; h.m_done = p->m_done; h.head_cap = p->eng.head_cap; h.hist_n = p->eng.hist_n;
    h.pending = (int64_t)p->eng.pending();
    h.last_re = p->last_re; h.last_im = p->last_im;
    if (p->has_dev_state()) {
        SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));
        SDRHIP_CHECK_HIP(hipMemcpy(h.dc, p->dc_state.p, 16, hipMemcpyDeviceToHost));
    }
    const size_t need = pipe_state_header_bytes(p) + p->eng.state_bytes(h.hist_n, h.pending) + (size_t)h.n_blocks * sizeof(int32_t) +
                        pipe_state_am_bytes(p);
    if (capacity < need) {
        set_error("sdrhip_pipe_save: %zu bytes needed, %zu given", need, capacity);
        return SDRHIP_ERR_ARG;
    }
    memcpy(buf, &h, sizeof h);
    if (h.version == 2) {
        const PipeStateRows x = {p->rows(), (int32_t)p->fmt};
        memcpy((unsigned char*)buf + sizeof h, &x, sizeof x);
    }
    unsigned char* o = p->eng.save((unsigned char*)buf + pipe_state_header_bytes(p));
    for (int len : p->demod_blocks) { const int32_t v = len; memcpy(o, &v, sizeof v); o += sizeof v; }
    const PipeAmRecord am = pipe_state_am(p);
    if (am.present) {
        // the flush above has harvested every submission, so the floats on the device -- dcBlocker's pairs (as the dcBlocker Pipe's
        // save), or the array the last fmDemod-form launch wrote -- are the stream's
        memcpy(o, &am.x, sizeof am.x);
        o += sizeof am.x;
        if (am.x.n_floats > 0) {
            SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));
            SDRHIP_CHECK_HIP(hipMemcpy(o, am.d_floats, (size_t)am.x.n_floats * sizeof(float), hipMemcpyDeviceToHost));
            o += (size_t)am.x.n_floats * sizeof(float);
        }
    }
    if (p->tail) {
        PipeStateAudio x = {p->a_done, p->y_n, {0, 0, 0, 0}};
        (void)sdrhip_audio_tail_shape(p->tail, x.shape);
        memcpy(o, &x, sizeof x);
        o += sizeof x;
        if (p->y_n > 0) {
            SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));
            SDRHIP_CHECK_HIP(hipMemcpy2D(o, (size_t)p->y_n * sizeof(float), p->y_rows[p->y_cur].p, (size_t)p->y_stride * sizeof(float),
                                         (size_t)p->y_n * sizeof(float), (size_t)p->rows(), hipMemcpyDeviceToHost));
        }
    }
    if (p->narrow) {
        const PipeStateNarrow x = pipe_state_narrow(p);
        memcpy(o, &x, sizeof x);
        o += sizeof x;
        SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));
        if (x.n_floats > 0) {
            SDRHIP_CHECK_HIP(hipMemcpy(o, pipe_narrow_floats(p), (size_t)x.n_floats * sizeof(float), hipMemcpyDeviceToHost));
            o += (size_t)x.n_floats * sizeof(float);
        }
        if (p->y_n > 0)
            SDRHIP_CHECK_HIP(hipMemcpy2D(o, (size_t)p->y_n * 2 * sizeof(float), p->y_rows[p->y_cur].p, (size_t)p->y_stride * sizeof(float),
                                         (size_t)p->y_n * 2 * sizeof(float), (size_t)p->rows(), hipMemcpyDeviceToHost));
    }
    *used = need;
    return SDRHIP_OK;
}

int sdrhip_pipe_restore(sdrhip_pipe* p, const void* buf, size_t bytes)
{
    if (p != nullptr && p->kind == PK_SPECTRUM) {
        SDRHIP_REQUIRE(buf != nullptr && bytes >= 3 * sizeof(int32_t), "sdrhip_pipe_restore");
        SDRHIP_REQUIRE(p->eng.pushes == 0 && p->sp_pos == 0 && p->eng.staged == 0 && p->eng.pending() == 0,
                       "sdrhip_pipe_restore: only into a pipe that has not been pushed to");
        PipeStateSpectrum x;
        memset(&x, 0, sizeof x);
        memcpy(&x, buf, bytes < sizeof x ? bytes : sizeof x);
        SDRHIP_REQUIRE(x.magic == kPipeMagic, "sdrhip_pipe_restore: not a pipe state");
        SDRHIP_REQUIRE(x.version == kPipeSpectrumVersion && x.kind == (int32_t)PK_SPECTRUM, "sdrhip_pipe_restore: the state belongs to a pipe of another kind");
        SDRHIP_REQUIRE(bytes >= sizeof x, "sdrhip_pipe_restore: truncated state");
        SDRHIP_REQUIRE(x.n == p->block_out && x.input_type == (int32_t)p->fmt && x.hop == p->sp_hop && x.group == p->sp_group && x.reduce == p->sp_reduce &&
                           x.unit == p->sp_unit && memcmp(&x.floor_db, &p->sp_floor_db, sizeof(double)) == 0,
                       "sdrhip_pipe_restore: the state belongs to a waterfall pipe of other parameters");
        // the tail holds no whole row and starts where row rows_done does
        const __int128 start = (__int128)x.rows_done * p->sp_group * p->sp_hop;
        SDRHIP_REQUIRE(x.pos >= 0 && x.rows_done >= 0 && x.skip >= 0 && x.tail_n >= 0 && x.pending >= 0 && x.pending % p->block_out == 0 &&
                           x.tail_n <= p->eng.head_cap && (x.skip == 0 || x.tail_n == 0) && start == (__int128)x.pos - x.tail_n + x.skip &&
                           spectrum_rows_in(p, x.tail_n) == 0,
                       "sdrhip_pipe_restore: inconsistent state");
        SDRHIP_REQUIRE(x.pending <= (int64_t)((bytes - sizeof x) / sizeof(float)) &&
                           bytes - sizeof x >= p->eng.state_bytes(x.tail_n, x.pending), "sdrhip_pipe_restore: truncated state");
        (void)p->eng.restore((const unsigned char*)buf + sizeof x, x.tail_n, x.pending);
        p->sp_pos = x.pos; p->sp_rows_done = x.rows_done; p->sp_skip = x.skip;
        return ready_blocks(p);
    }
    SDRHIP_REQUIRE(p != nullptr && buf != nullptr && bytes >= sizeof(PipeStateHeader), "sdrhip_pipe_restore");
    SDRHIP_REQUIRE(p->eng.pushes == 0 && p->E_prev == 0 && p->eng.staged == 0 && p->eng.pending() == 0,
                   "sdrhip_pipe_restore: only into a pipe that has not been pushed to");
    PipeStateHeader h;
    memcpy(&h, buf, sizeof h);
    SDRHIP_REQUIRE(h.magic == kPipeMagic && (h.version == 1 || h.version == 2), "sdrhip_pipe_restore: not a pipe state");
    SDRHIP_REQUIRE(h.version == pipe_state_version(p), "sdrhip_pipe_restore: the state belongs to a pipe of another row count or input type");
    if (h.version == 2) {
        SDRHIP_REQUIRE(bytes >= pipe_state_header_bytes(p), "sdrhip_pipe_restore: truncated state");
        PipeStateRows x;
        memcpy(&x, (const unsigned char*)buf + sizeof h, sizeof x);
        SDRHIP_REQUIRE(x.rows == p->rows() && x.input_u8 == (int32_t)p->fmt,
                       "sdrhip_pipe_restore: the state belongs to a pipe of another row count or input type");
    }
    SDRHIP_REQUIRE(h.kind == (int32_t)p->kind && h.block_out == p->block_out && h.I == p->I && h.D == p->D && h.Lp == p->Lp &&
                       h.cplx_in == (int32_t)p->cplx_in && h.cplx_out == (int32_t)p->cplx_out && h.head_cap == p->eng.head_cap,
                   "sdrhip_pipe_restore: the state belongs to a pipe of another kind or geometry");
    SDRHIP_REQUIRE(h.hist_n >= 0 && h.hist_n <= h.head_cap && h.pending >= 0 && h.n_blocks >= 0 && h.E_prev >= h.hist_n && h.m_done >= 0,
                   "sdrhip_pipe_restore: inconsistent state");
    if (p->kind == PK_FILTER || p->kind == PK_DECIMATOR || p->kind == PK_RESAMPLER || p->kind == PK_TUNER || p->kind == PK_TUNER_BANK ||
        p->am_kind() || p->nfm_kind() || p->kind == PK_NARROW_BANK) {
        // the next pending output must start inside what the pipe has seen, every output computable from those elements must be
        // done at most once, and the history must reach back to its first input (3 elements of alignment slack, 7 of u8, fir_submit):
        // otherwise the kernels would be sent in front of the staging buffer
        const int64_t first_in = p->in_offset(h.m_done);
        const int64_t m_max = (h.E_prev * p->I >= p->Lp) ? (h.E_prev * p->I - p->Lp) / p->D + 1 : 0;
        int64_t keep_from = first_in < h.E_prev ? first_in : h.E_prev;
        keep_from -= keep_from & (p->tail_align() - 1);
        SDRHIP_REQUIRE(h.m_done <= m_max && first_in <= h.E_prev + (p->Lp + p->D) / p->I + 1 && h.hist_n >= h.E_prev - keep_from,
                       "sdrhip_pipe_restore: the position and the history of the state do not belong together");
    }
    const size_t am_at = pipe_state_header_bytes(p) + p->eng.state_bytes(h.hist_n, h.pending) + (size_t)h.n_blocks * sizeof(int32_t);
    const PipeAmRecord am = pipe_state_am(p);
    SDRHIP_REQUIRE(bytes >= am_at + am.bytes() + (p->tail ? sizeof(PipeStateAudio) : 0) + (p->narrow ? sizeof(PipeStateNarrow) : 0),
                   "sdrhip_pipe_restore: truncated state");
    if (am.present) {
        PipeStateAm x;
        memcpy(&x, (const unsigned char*)buf + am_at, sizeof x);
        SDRHIP_REQUIRE(x.dc_block == am.x.dc_block && x.n_floats == am.x.n_floats,
                       p->am_kind() ? "sdrhip_pipe_restore: the state belongs to an AM bank pipe of another dc_block"
                                    : "sdrhip_pipe_restore: the state belongs to a pipe of another row count");
    }
    PipeStateAudio au = {0, 0, {0, 0, 0, 0}};
    const unsigned char* au_floats = nullptr;
    if (p->tail) {
        int32_t shape[4];
        memcpy(&au, (const unsigned char*)buf + am_at + am.bytes(), sizeof au);
        (void)sdrhip_audio_tail_shape(p->tail, shape);
        SDRHIP_REQUIRE(memcmp(au.shape, shape, sizeof shape) == 0,
                       "sdrhip_pipe_restore: the state belongs to an audio pipe of another resampler ratio or other tail tap counts");
        // every audio output the demodulated outputs so far complete is done, and the carried rows reach back to the next one's first input
        SDRHIP_REQUIRE(au.a_done == sdrhip_audio_tail_ready(p->tail, h.m_done) && au.y_n >= 0 && au.y_n <= h.m_done &&
                           sdrhip_audio_tail_first_input(p->tail, au.a_done) >= h.m_done - au.y_n &&
                           au.y_n <= h.m_done - sdrhip_audio_tail_first_input(p->tail, au.a_done) + sdrhip_audio_tail_max_halo(p->tail),
                       "sdrhip_pipe_restore: inconsistent state");
        SDRHIP_REQUIRE((bytes - (am_at + am.bytes() + sizeof au)) / sizeof(float) >= (size_t)p->rows() * (size_t)au.y_n,
                       "sdrhip_pipe_restore: truncated state");
        au_floats = (const unsigned char*)buf + am_at + am.bytes() + sizeof au;
    }
    PipeStateNarrow nx;
    memset(&nx, 0, sizeof nx);
    const unsigned char* nx_floats = nullptr;
    if (p->narrow) {
        memcpy(&nx, (const unsigned char*)buf + am_at, sizeof nx);
        const PipeStateNarrow mine = pipe_state_narrow(p);
        SDRHIP_REQUIRE(nx.block_mid == mine.block_mid, "sdrhip_pipe_restore: the state belongs to a narrow bank pipe of another block_mid");
        SDRHIP_REQUIRE(nx.D2 == mine.D2 && nx.Lp2 == mine.Lp2,
                       "sdrhip_pipe_restore: the state belongs to a narrow bank pipe of another second decimator (factor or tap count)");
        SDRHIP_REQUIRE(nx.form == mine.form && nx.dc_block == mine.dc_block && nx.n_floats == mine.n_floats,
                       "sdrhip_pipe_restore: the state belongs to a narrow bank pipe of another form, dc_block or row count");
        // every stage-2 output the whole blocks of stage-1 outputs so far complete is done, and the carried rows reach back to the
        // next one's first input
        const int64_t first = nx.a_done * (int64_t)mine.D2;
        SDRHIP_REQUIRE(nx.a_done == p->narrow_ready(h.m_done) && nx.y_n >= 0 && nx.y_n <= h.m_done && (first >= h.m_done || nx.y_n >= h.m_done - first),
                       "sdrhip_pipe_restore: inconsistent state");
        SDRHIP_REQUIRE((bytes - (am_at + sizeof nx)) / sizeof(float) >= (size_t)nx.n_floats + (size_t)p->rows() * (size_t)nx.y_n * 2,
                       "sdrhip_pipe_restore: truncated state");
        nx_floats = (const unsigned char*)buf + am_at + sizeof nx;
    }
    // (the one step that can fail for want of memory comes before anything is put back: a failed restore leaves the pipe fresh)
    if (p->rows_tail()) {
        int rc = audio_rows_room(p, (p->narrow ? nx.y_n : au.y_n) + 1, p->eng.compute[0]);
        if (rc != SDRHIP_OK) return rc;
    }
    const unsigned char* in = p->eng.restore((const unsigned char*)buf + pipe_state_header_bytes(p), h.hist_n, h.pending);
    p->E_prev = h.E_prev;
    p->m_done = h.m_done;
    p->uniform_n = h.uniform_n;
    p->all_uniform = h.all_uniform != 0;
    p->last_re = h.last_re;
    p->last_im = h.last_im;
    p->demod_blocks.clear();
    for (int i = 0; i < h.n_blocks; i++) { int32_t v; memcpy(&v, in, sizeof v); in += sizeof v; p->demod_blocks.push_back(v); }
    if (am.x.n_floats > 0) {
        SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));       // the create call's memsets
        SDRHIP_CHECK_HIP(hipMemcpy(am.d_floats, in + sizeof(PipeStateAm), (size_t)am.x.n_floats * sizeof(float), hipMemcpyHostToDevice));
    }
    if (p->has_dev_state()) {
        SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));       // the create call's memset
        SDRHIP_CHECK_HIP(hipMemcpy(p->dc_state.p, h.dc, 16, hipMemcpyHostToDevice));
    }
    if (p->tail) {
        p->a_done = au.a_done;
        if (au.y_n > 0)
            SDRHIP_CHECK_HIP(hipMemcpy2D(p->y_rows[p->y_cur].p, (size_t)p->y_stride * sizeof(float), au_floats, (size_t)au.y_n * sizeof(float),
                                         (size_t)au.y_n * sizeof(float), (size_t)p->rows(), hipMemcpyHostToDevice));
        p->y_n = au.y_n;
    }
    if (p->narrow) {
        SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));       // the create call's memsets
        if (nx.n_floats > 0)
            SDRHIP_CHECK_HIP(hipMemcpy(pipe_narrow_floats(p), nx_floats, (size_t)nx.n_floats * sizeof(float), hipMemcpyHostToDevice));
        p->a_done = nx.a_done;
        if (nx.y_n > 0)
            SDRHIP_CHECK_HIP(hipMemcpy2D(p->y_rows[p->y_cur].p, (size_t)p->y_stride * sizeof(float), nx_floats + (size_t)nx.n_floats * sizeof(float),
                                         (size_t)nx.y_n * 2 * sizeof(float), (size_t)nx.y_n * 2 * sizeof(float), (size_t)p->rows(),
                                         hipMemcpyHostToDevice));
        p->y_n = nx.y_n;
    }
    return ready_blocks(p);
}

void sdrhip_pipe_destroy(sdrhip_pipe* p)
{
    // the borrowed spectrum object outlives the pipe's streams: it must not remember one of them as its scratch's last user
    if (p != nullptr && p->kind == PK_SPECTRUM)
        for (hipStream_t st : p->eng.compute)
            if (st) spectrum_forget_stream(p->spec, st);
    delete p;
}

}  // extern "C"
