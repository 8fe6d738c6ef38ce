// pipe.hpp -- private to pipes*.cpp: the kind table, struct sdrhip_pipe and its parts, the few helpers more than one of the files needs.
//   pipes.cpp           the create calls, push / pop / poll / flush / input_buffer / set_*, destroy, the map stages
//   pipes_fir.cpp       the FIR-like stages and the banks: fir_like_push, fir_submit and the rows tail
//   pipes_spectrum.cpp  the waterfall Pipe and its state record
//   pipes_state.cpp     sdrhip_pipe_state_bytes / _save / _restore: the saved-state layout, stated once
#pragma once
#include <stdlib.h>
#include <string.h>

#include <deque>

#include "am.hpp"
#include "descriptors.hpp"
#include "host_stream.hpp"
#include "spectrum.hpp"

using namespace sdrhip;
#define PIPE_LOCAL __attribute__((visibility("hidden")))      // what the files share stays out of the library's symbol table

// The one kind table.  Saved states in the field hold these numbers: a new kind takes the NEXT number, and no number is ever reused.
enum PipeKind : int {
    PK_FILTER = 0, PK_DECIMATOR = 1, PK_RESAMPLER = 2, PK_DEMOD = 3, PK_DCBLOCK = 4, PK_AGC = 5, PK_TUNER = 6, PK_TUNER_BANK = 7, PK_AM = 8,
    PK_AM_BANK = 9, PK_SPECTRUM = 10, PK_NFM_BANK = 11, PK_AM_BANK_AUDIO = 12, PK_NFM_BANK_AUDIO = 13, PK_NARROW_BANK = 14,
};

// room for `bytes` in a scratch buffer that launches already on stream s may still use: growing frees the old buffer, so they end first
static inline int grow(DevBuf& b, size_t bytes, hipStream_t s)
{
    if (bytes > b.cap) SDRHIP_CHECK_HIP(hipStreamSynchronize(s));
    return b.ensure(bytes);
}

// One pair of floats per channel on the device, which a chain of launches reads and writes.  Ping-pong (fmDemod's last decimated
// sample): a launch reads latest() and writes out(), the other array -- the two must not overlap, kernels_tuner_bank.hip -- and the host
// flips after every launch, so consecutive launches depend on each other through it.  In place (dcBlocker's pairs): out() == latest().
struct PIPE_LOCAL ChannelState {
    DevBuf buf[2];
    int cur = 0;
    bool pingpong = false;
    float* latest() const { return (float*)buf[cur].p; }        // what the next launch reads: the stream's state between submissions
    float* out() const { return (float*)buf[pingpong ? cur ^ 1 : cur].p; }
    void ran() { if (pingpong) cur ^= 1; }
};

// The device rows behind a bank part (the audio Pipes, the narrow Pipe): K rows of `stride` floats in rows[cur], elements of `width`
// floats, the first n of every row carried from earlier submissions; a_done outputs of the stage behind the rows are done.
struct PIPE_LOCAL RowsCarry {
    DevBuf rows[2], ws;            // ws: the workspace of the run behind the rows
    int cur = 0, width = 1;
    int64_t stride = 0, n = 0, a_done = 0;
    float* data() const { return (float*)rows[cur].p; }
    size_t pitch() const { return (size_t)stride * sizeof(float); }
    size_t span(int64_t count) const { return (size_t)(count * width) * sizeof(float); }      // bytes of `count` elements of one row
    // Room for `need` elements per row in both buffers.  Growing (the first submission, or a larger push than any before) waits for the
    // launches on s that still use the old buffers and moves the n carried elements of every row over.
    int room(int K, int64_t need, hipStream_t s)
    {
        need *= width;
        if (need <= stride) return SDRHIP_OK;
        const int64_t wider = row_floats(need + need / 4 + 512);
        DevBuf bigger[2];
        int rc;
        for (DevBuf& b : bigger)
            if ((rc = b.ensure((size_t)K * (size_t)wider * sizeof(float))) != SDRHIP_OK) return rc;
        SDRHIP_CHECK_HIP(hipStreamSynchronize(s));
        if (n > 0)
            SDRHIP_CHECK_HIP(hipMemcpy2D(bigger[0].p, (size_t)wider * sizeof(float), data(), pitch(), span(n), (size_t)K, hipMemcpyDeviceToDevice));
        for (int i = 0; i < 2; i++) {
            std::swap(rows[i].p, bigger[i].p);
            std::swap(rows[i].cap, bigger[i].cap);
        }
        cur = 0; stride = wider;
        return SDRHIP_OK;
    }
    // the carry step: the last `keep` (clamped to 0 .. n_y) of the n_y elements go to the front of the other buffer, on stream s
    int carry(int K, int64_t n_y, int64_t keep, hipStream_t s)
    {
        keep = keep < 0 ? 0 : keep > n_y ? n_y : keep;
        if (keep > 0)
            SDRHIP_CHECK_HIP(hipMemcpy2DAsync(rows[cur ^ 1].p, pitch(), data() + width * (n_y - keep), pitch(), span(keep), (size_t)K,
                                              hipMemcpyDeviceToDevice, s));
        cur ^= 1; n = keep;
        return SDRHIP_OK;
    }
    // the carried rows of a saved state, K * count elements row after row: out of rows[cur] (a save) or into it (a restore, behind room())
    int host_copy(int K, void* host, int64_t count, hipMemcpyKind kind) const
    {
        const bool out = kind == hipMemcpyDeviceToHost;
        if (count > 0)
            SDRHIP_CHECK_HIP(hipMemcpy2D(out ? host : data(), out ? span(count) : pitch(), out ? data() : host, out ? pitch() : span(count),
                                         span(count), (size_t)K, kind));
        return SDRHIP_OK;
    }
};

// PK_SPECTRUM: the waterfall Pipe over a borrowed spectrum object.  Elements are samples in the object's own type (fmt); output
// blocks are rows of block_out = n floats.  The engine's history holds exactly the carried tail (the samples from the first row
// not yet produced onward) while nothing is staged; skip samples of the stream are still to be dropped on arrival (hop > n).
struct PIPE_LOCAL SpectrumPart {
    sdrhip_spectrum* spec = nullptr;
    int64_t hop = 0, pos = 0, rows_done = 0, skip = 0;      // pos: samples pushed so far
    int group = 1, reduce = 0, unit = 0;
    double floor_db = 0.0;
};

// What fir_submit does with a submission: decided once by the create call (pipes.cpp), only read afterwards.
struct PIPE_LOCAL PipePolicy {
    // every launch on compute stream 0, whatever the slot: the submissions depend on each other through state on the device, and the
    // stream orders them.  Set by: AM bank with dc_block, NFM bank, both audio Pipes, the narrow bank
    bool stream0 = false;
    // submissions up to kDirectBytes read the pinned staging buffer in place.  Cleared by: every bank of more than one row (with K
    // channels in the grid every channel's workgroups would fetch the same tile over the link: the reason the FM bank's stream gives,
    // chain.cpp) and the AM / NFM kinds even with one row (a stated choice: the FM bank stream's sweep found no in-place region)
    bool in_place = true;
    // a copied submission is placed so that the banked launch's first window is 16-byte aligned (HostStream::dev_skew).  Set by: every bank
    bool align_first = false;
    // complex scratch rows for EVERY submission, not only for those whose tile part the fused launch does not take.  Set by: the AM
    // kinds (whether the fused launch takes a submission is left to the launcher there)
    bool iq_always = false;
};

struct sdrhip_pipe {
    PipeKind kind;
    const FirDesc* fir = nullptr;
    const ResampDesc* rs = nullptr;
    const TunerDesc* tuner = nullptr;  // PK_TUNER: the decimator behind the oscillator mix (fir = &tuner->fir)
    int block_out = 0;
    bool cplx_in = false, cplx_out = false;
    int I = 1, D = 1, Lp = 1;
    InFmt fmt = IN_CF32;               // cfloat, interleaved u8 IQ or interleaved int16 IQ blocks, which stay so up to the kernels' loaders
    PipePolicy pol;
    // ---- the bank Pipes: every channel of the bank in lockstep, one output row per channel (the engine's rows); fir = channel 0's
    // decimator, which is every channel's.  form: the output form (descriptors.hpp) -- IQ (tuner bank; the narrow bank's stage 1), ENV
    // (the AM kinds: ONE float per output, the envelope), PHASE (the NFM kinds: fmDemod of each channel over the whole stream).
    const TunerBankDesc* bank = nullptr;
    BankForm::Kind form = BankForm::IQ;
    // complex rows of a submission the fused launch does not serve (another order or factor), one buffer per slot because without
    // pol.stream0 the slots' submissions run on streams of their own
    DevBuf iq_scratch[HostStream::kMaxSlots];
    // fm: every channel's last decimated output (the NFM kinds; the narrow bank's FM form).  dc: dcBlocker's pairs (am_dc: the AM kinds
    // with dc_block, whose envelope rows and dcBlocker workspace are dc_ws; the narrow bank's envelope form with dc_block)
    ChannelState fm, dc;
    bool am_dc = false;
    DevBuf dc_ws;
    // ---- the rows tails: a stage behind the bank part, on the device rows y.  The bank part of a submission writes its rows into y
    // behind the y.n elements carried from earlier submissions (row element 0 is bank output m_done - y.n of the stream), ONE run then
    // computes the tail's outputs [y.a_done, tail_ready(m_end)) into the chunk, and the rest is carried (rows_tail, pipes_fir.cpp).
    // tail: PK_AM_BANK_AUDIO / PK_NFM_BANK_AUDIO, a BORROWED sdrhip_audio_tail behind the demodulated rows; block_out is the tail's block.
    // narrow: PK_NARROW_BANK, a BORROWED sdrhip_narrow_bank whose stage 2 (second decimator, demodulator, dcBlocker) runs behind the
    // COMPLEX stage-1 rows with seam_block2 = block_mid -- it sees whole blocks of block_mid only, as the second firDecimator behind
    // `firDecimator deci1 block_mid` does; block_out is the Pipe's own output block.
    const sdrhip_audio_tail* tail = nullptr;
    const NarrowBankDesc* narrow = nullptr;
    int64_t block_mid = 0;
    // narrow AND tail (sdrhip_pipe_narrow_bank_audio, still PK_NARROW_BANK): stage 2 writes its real rows behind the carried history of a
    // SECOND carry, y2, instead of into the chunk, one sdrhip_audio_tail_run_rows computes the audio outputs [y2.a_done, audio_ready)
    // into the chunk, then both carries step.  y2's row element 0 is stage-2 output (y.a_done - y2.n) of the stream; block_out is the
    // tail's block.
    RowsCarry y, y2;
    bool rows_tail() const { return tail != nullptr || narrow != nullptr; }
    bool narrow_audio() const { return tail != nullptr && narrow != nullptr; }
    // floats per row a submission leaves in the chunk once a_end outputs of the (first) rows tail are done, and with it the audio position
    int64_t chunk_outputs(int64_t a_end, int64_t* q_end) const
    {
        if (!narrow_audio()) return a_end - y.a_done;
        *q_end = std::max(y2.a_done, sdrhip_audio_tail_ready(tail, a_end));
        return *q_end - y2.a_done;
    }
    // what the two rows tails differ in besides their run: outputs ready after m bank outputs, first bank output that output a needs
    int64_t tail_ready(int64_t m) const
    {
        if (!narrow) return sdrhip_audio_tail_ready(tail, m);
        const int64_t n1 = m / block_mid * block_mid;
        return n1 >= narrow->d2->Lp ? (n1 - narrow->d2->Lp) / narrow->d2->factor + 1 : 0;
    }
    int64_t tail_first_input(int64_t a) const { return narrow ? a * narrow->d2->factor : sdrhip_audio_tail_first_input(tail, a); }
    SpectrumPart sp;

    // Four slots = submissions in flight (round 3; SDRHIP_STREAM_SLOTS=2..4).  An in-place push of one host block is one small
    // kernel, ~20 us of latency end to end over PCIe, and the host is done submitting it in ~6: the slots keep the GPU fed.
    bool direct_ok = stream_knobs().direct;
    static constexpr size_t kDirectBytes = 512 << 10;     // [tail | staged] up to this size is read in place over PCIe
    static constexpr size_t kAdaptiveBytes = 4 << 20;     // adaptive submission stages at most this much
    int64_t E_prev = 0;     // global end of the previous block
    int64_t m_done = 0;     // outputs computed so far
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
    // (FIR-like stages) make the current slot writable with room for `elems` staged elements: growth keeps what is staged and the lent ones
    int open_slot(size_t elems) { return eng.open_slot(elems * ein(), (size_t)(eng.staged + lent) * ein()); }
    // ---- the map stages (one row): fmDemod's carry (Demod.hs:41,46); dcBlockingFilter's {lastSample, lastOutput} / agcPipe's {state}
    // carried on the device in map_state (16 bytes), their launches' workspace in map_ws
    float last_re = 0.0f, last_im = 0.0f;
    std::deque<int> demod_blocks;      // output block lengths (one per input block)
    DevBuf map_state, map_ws;
    float agc_mu = 0.0f, agc_ref = 0.0f;
    // PK_DCBLOCK's second form (sdrhip_pipe_deemph): not 0 = a de-emphasis pipe of this alpha, whose map_state is {y, 0, alpha, 0}
    float deemph_alpha = 0.0f;
    bool is_map() const { return kind == PK_DEMOD || kind == PK_DCBLOCK || kind == PK_AGC || kind == PK_AM; }

    int esz_in() const { return cplx_in ? 2 : 1; }
    size_t ein() const { return fmt == IN_U8 ? 2 : fmt == IN_I16 ? 4 : (size_t)esz_in() * 4; }      // bytes per input element
    // the carried tail starts at a multiple of this many elements: 16 bytes of u8 or int16 input (and the 4 every float pipe always had)
    int64_t tail_align() const { return fmt == IN_U8 ? 8 : 4; }
    int rows() const { return eng.rows; }
    int esz_out() const { return cplx_out ? 2 : 1; }
    int64_t in_offset(int64_t m) const { return ceil_div64(m * (int64_t)D, I); }
    // outputs_by(E): outputs computable once E elements are in (window end <= E*I).  keep_from(m, E): where the carried tail starts with
    // m outputs done -- the first input any pending output needs, rounded down to a multiple of tail_align() (16-byte aligned device reads)
    int64_t outputs_by(int64_t E) const { return E * I >= Lp ? (E * I - Lp) / D + 1 : 0; }
    int64_t keep_from(int64_t m, int64_t E) const { return std::min(in_offset(m), E) & ~(tail_align() - 1); }
    // Elements of esz_in() floats; head room for the carried tail of FIR-like pipes.  Declared last: destroyed first, so its
    // streams are idle before the device buffers above are freed.
    HostStream eng;
};

// A pipe of the given kind and geometry, with its engine: FIR-like pipes get head room and history for the carried tail,
// E_prev - in_offset(m_done) < (Lp + D) / I + 1 elements, plus up to 3 of alignment slack (7 of a u8 pipe); map pipes carry nothing; the
// waterfall Pipe says what it carries (head_cap >= 0).
PIPE_LOCAL int pipe_new(sdrhip_pipe** out, PipeKind kind, const FirDesc* fir, const ResampDesc* rs, int block_out, bool cplx_in, bool cplx_out,
                        int I, int D, int Lp, InFmt fmt = IN_CF32, int64_t head_cap = -1);
// A pipe's state on the device: `bytes` of `buf` (at least 16), zeros -- set on the first compute stream -- or a copy of `init`.  On
// failure the pipe is destroyed and *pp is null.
PIPE_LOCAL int pipe_dev_state(sdrhip_pipe** pp, DevBuf& buf, size_t bytes, const void* init, const char* who);
PIPE_LOCAL int ready_blocks(const sdrhip_pipe* p);
PIPE_LOCAL int fir_like_push(sdrhip_pipe* p, const void* block, int n);
PIPE_LOCAL int fir_submit(sdrhip_pipe* p, int n, int64_t uniform_seam);
PIPE_LOCAL int spectrum_push(sdrhip_pipe* p, const void* block, int n);
PIPE_LOCAL int spectrum_open_slot(sdrhip_pipe* p, int64_t elems);
PIPE_LOCAL int spectrum_settle(sdrhip_pipe* p);
PIPE_LOCAL size_t spectrum_state_bytes(const sdrhip_pipe* p);
PIPE_LOCAL int spectrum_save(sdrhip_pipe* p, void* buf);
PIPE_LOCAL int spectrum_restore(sdrhip_pipe* p, const void* buf, size_t bytes);
constexpr uint32_t kPipeMagic = 0x50504453u;   // "SDPP": the first word of every saved state
