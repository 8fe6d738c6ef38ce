// pipes_state.cpp -- checkpoint / resume (as sdrhip_fm_stream_save / _restore, chain.cpp): sdrhip_pipe_state_bytes, _save, _restore.
// Between two pushes a Pipe's state is its position (elements consumed, outputs produced), the last head_cap input elements,
// the carried fmDemod sample / dcBlocker pair / agc state, and the output not yet popped: what the reference keeps in the Pipe's closure
// (Filter.hs:536-727: overlap remainder, resampler (group, offset); Demod.hs:41,46; Filter.hs:730-739).
//
// THE LAYOUT, stated here once.  A version 1 or 2 state is these records, in this order:
//   1. PipeStateHeader
//   2. PipeStateRows                   version 2 only: a pipe of more than one row or of u8 / int16 input
//   3. the engine's history and fifo   HostStream::save: hist_n elements in the input's own type, then pending floats row after row
//   4. n_blocks int32 block lengths    the map stages' output blocks not yet popped
//   5. the bank record (the AM and NFM kinds)   6. the audio record (the audio Pipes)   7. the narrow record (the narrow bank's Pipe)
//   8. the audio record again, behind the narrow record: the narrow bank's Pipe with an audio tail (has_tail = 1 in record 7), whose
//      rows are the carried REAL stage-2 outputs of the second carry
// The header's dc[4] is the map stage's 16 bytes of device state as they stand: dcBlocker {lastSample, lastOutput, 0, 0}, agc {state, 0, 0,
// 0}, and de-emphasis (the one-pole map kind's second form: the header's kind is the dcBlocker's) {y, 0, alpha, 0}.  dc[2] as bits tells
// the two forms apart -- 0 = dcBlocker, whose states keep every byte they had -- and one alpha from another; restore compares it.
// Each of these trailing records is [a fixed part | n_floats floats of a ChannelState | a rows carry's K * y_n elements]: one Trailer
// says what this pipe writes as the fixed part, where the floats live, which carry's rows follow, and how a state's fixed part is
// checked against this pipe.  state_bytes, save and restore walk the same list (Trailers).  Version 3 (the waterfall) is a header of its own
// plus the engine's state: pipes_spectrum.cpp.
#include "pipe.hpp"

namespace {
struct PipeStateHeader {
    uint32_t magic, version;
    int32_t kind, block_out, I, D, Lp, cplx_in, cplx_out, uniform_n, all_uniform, n_blocks;
    int64_t E_prev, m_done, head_cap, hist_n, pending;       // hist_n: elements; pending: floats in the fifo
    float last_re, last_im, dc[4];
};
// Version 2: the same header, then this, then the engine's state with the history in the input's own type (2 bytes per u8 element, 4
// per int16 one) and the fifo row after row; input_u8 is the input type: 0 = cfloat, 1 = u8, 2 = int16.  Every other pipe writes
// version 1, byte for byte as before.
struct PipeStateRows { int32_t rows, input_u8; };
uint32_t pipe_state_version(const sdrhip_pipe* p) { return p->rows() > 1 || p->fmt != IN_CF32 ? 2u : 1u; }
size_t pipe_state_header_bytes(const sdrhip_pipe* p) { return sizeof(PipeStateHeader) + (pipe_state_version(p) == 2 ? sizeof(PipeStateRows) : 0); }
// 5. dc_block, the number of floats, the floats: the AM kinds' dcBlocker pairs (2 K with dc_block, else none: as the dcBlocker Pipe's
// save), or with dc_block = 0 the NFM kinds' last decimated (re, im) of every channel (2 K: the array the last fmDemod-form launch wrote)
struct PipeStateAm { int32_t dc_block, n_floats; };
// 6. the audio position, the tail's shape (so that a state is restored only into a pipe of the same resampler ratio and tap counts) and
// the y_n carried demodulated elements of every row, row after row.  Behind a narrow record (8.) the positions count in stage-2 outputs:
// y_n carried real stage-2 outputs of every row, a_done audio outputs done
struct PipeStateAudio {
    int64_t a_done, y_n;
    int32_t shape[4];        // sdrhip_audio_tail_shape: interpolation, decimation, numCoeffsR, numCoeffsF
};
// 7. the stage-2 position, what the state may be restored into (block_mid, the second decimator's factor and prepared length, the form,
// dc_block), n_floats state floats (fmDemod's pairs or dcBlocker's, 2 K; 0 for the plain envelope) and the y_n carried COMPLEX stage-1
// outputs of every row, row after row.  has_tail: 1 = an audio record follows (sdrhip_pipe_narrow_bank_audio); a plain narrow pipe writes
// the 0 the field always held
struct PipeStateNarrow {
    int64_t a_done, y_n, block_mid;
    int32_t D2, Lp2, form, dc_block, n_floats, has_tail;
};

struct Trailer {
    void* fixed;                  // the fixed part: as this pipe writes it; once check() has accepted a state's, that one
    size_t fixed_bytes;
    float* floats;                // the n_floats floats behind it, on the device
    int32_t n_floats;
    const int64_t* rows;          // {a_done, y_n} inside the fixed part where a rows carry's K * y_n elements follow, else null
    RowsCarry* carry;             // ... that carry
    int (*check)(const sdrhip_pipe* p, const unsigned char* in, const PipeStateHeader& h, void* mine);
    size_t bytes(const sdrhip_pipe* p) const
    {
        return fixed_bytes + (size_t)n_floats * sizeof(float) + (rows ? (size_t)p->rows() * carry->span(rows[1]) : 0);
    }
};

int check_bank(const sdrhip_pipe* p, const unsigned char* in, const PipeStateHeader&, void* fixed)
{
    const PipeStateAm& mine = *(const PipeStateAm*)fixed;
    PipeStateAm x;
    memcpy(&x, in, sizeof x);
    SDRHIP_REQUIRE(x.dc_block == mine.dc_block && x.n_floats == mine.n_floats,
                   p->form == BankForm::ENV ? "sdrhip_pipe_restore: the state belongs to an AM bank pipe of another dc_block"
                                            : "sdrhip_pipe_restore: the state belongs to a pipe of another row count");
    return SDRHIP_OK;
}

int check_audio(const sdrhip_pipe* p, const unsigned char* in, const PipeStateHeader& h, void* fixed)
{
    PipeStateAudio& mine = *(PipeStateAudio*)fixed;
    PipeStateAudio au;
    memcpy(&au, in, sizeof au);
    SDRHIP_REQUIRE(memcmp(au.shape, mine.shape, sizeof mine.shape) == 0,
                   "sdrhip_pipe_restore: the state belongs to an audio pipe of another resampler ratio or other tail tap counts");
    // every audio output the demodulated outputs so far complete is done, and the carried rows reach back to the next one's first input
    // (behind a narrow record the demodulated outputs are the stage-2 outputs, which check_narrow has tied to the header already)
    const int64_t m = p->narrow ? p->tail_ready(h.m_done) : h.m_done;
    SDRHIP_REQUIRE(au.a_done == sdrhip_audio_tail_ready(p->tail, m) && au.y_n >= 0 && au.y_n <= m &&
                       sdrhip_audio_tail_first_input(p->tail, au.a_done) >= m - au.y_n &&
                       au.y_n <= m - sdrhip_audio_tail_first_input(p->tail, au.a_done) + sdrhip_audio_tail_max_halo(p->tail),
                   "sdrhip_pipe_restore: inconsistent state");
    mine = au;
    return SDRHIP_OK;
}

int check_narrow(const sdrhip_pipe* p, const unsigned char* in, const PipeStateHeader& h, void* fixed)
{
    PipeStateNarrow& mine = *(PipeStateNarrow*)fixed;
    PipeStateNarrow nx;
    memcpy(&nx, in, sizeof nx);
    SDRHIP_REQUIRE(nx.has_tail == mine.has_tail, mine.has_tail ? "sdrhip_pipe_restore: the state belongs to a narrow bank pipe without an audio tail"
                                                               : "sdrhip_pipe_restore: the state belongs to a narrow bank pipe with an audio tail");
    SDRHIP_REQUIRE(nx.block_mid == mine.block_mid, "sdrhip_pipe_restore: the state belongs to a narrow bank pipe of another block_mid");
    SDRHIP_REQUIRE(nx.D2 == mine.D2 && nx.Lp2 == mine.Lp2,
                   "sdrhip_pipe_restore: the state belongs to a narrow bank pipe of another second decimator (factor or tap count)");
    SDRHIP_REQUIRE(nx.form == mine.form && nx.dc_block == mine.dc_block && nx.n_floats == mine.n_floats,
                   "sdrhip_pipe_restore: the state belongs to a narrow bank pipe of another form, dc_block or row count");
    // every stage-2 output the whole blocks of stage-1 outputs so far complete is done, and the carried rows reach back to the
    // next one's first input
    const int64_t first = nx.a_done * (int64_t)mine.D2;
    SDRHIP_REQUIRE(nx.a_done == p->tail_ready(h.m_done) && nx.y_n >= 0 && nx.y_n <= h.m_done && (first >= h.m_done || nx.y_n >= h.m_done - first),
                   "sdrhip_pipe_restore: inconsistent state");
    mine = nx;
    return SDRHIP_OK;
}

// the trailing records of this pipe, in the order of the layout (t[] points into the object: it is not to be copied)
struct Trailers {
    PipeStateAm am;
    PipeStateAudio au;
    PipeStateNarrow nx;
    Trailer t[3];
    int n = 0;
    Trailers(const Trailers&) = delete;
    explicit Trailers(const sdrhip_pipe* p)
    {
        const RowsCarry& y = p->y;
        const bool nfm = p->form == BankForm::PHASE;
        if (p->form != BankForm::IQ) {
            am = {p->am_dc ? 1 : 0, p->am_dc || nfm ? 2 * p->rows() : 0};
            t[n++] = {&am, sizeof am, (nfm ? p->fm : p->dc).latest(), am.n_floats, nullptr, nullptr, check_bank};
        }
        RowsCarry* const first = const_cast<RowsCarry*>(&p->y);
        RowsCarry* const audio = p->narrow ? const_cast<RowsCarry*>(&p->y2) : first;      // the carry in front of the audio tail
        if (p->tail && !p->narrow) audio_record(p, audio);
        if (const NarrowBankDesc* nb = p->narrow) {
            const bool fm = nb->form == NARROW_FM;
            nx = {y.a_done, y.n, p->block_mid, nb->d2->factor, nb->d2->Lp, nb->form, nb->dc_block, fm || nb->dc_block ? 2 * p->rows() : 0,
                  p->tail ? 1 : 0};
            t[n++] = {&nx, sizeof nx, (fm ? p->fm : p->dc).latest(), nx.n_floats, &nx.a_done, first, check_narrow};
            if (p->tail) audio_record(p, audio);
        }
    }
    void audio_record(const sdrhip_pipe* p, RowsCarry* carry)
    {
        au = {carry->a_done, carry->n, {0, 0, 0, 0}};
        (void)sdrhip_audio_tail_shape(p->tail, au.shape);
        t[n++] = {&au, sizeof au, nullptr, 0, &au.a_done, carry, check_audio};
    }
    Trailer* begin() { return t; }
    Trailer* end() { return t + n; }
};

// records 1 - 4 with these counts, and the whole state of the (drained) pipe
size_t pipe_state_front_bytes(const sdrhip_pipe* p, int64_t hist_n, int64_t pending, int64_t n_blocks)
{
    return pipe_state_header_bytes(p) + p->eng.state_bytes(hist_n, pending) + (size_t)n_blocks * sizeof(int32_t);
}
size_t pipe_state_size(const sdrhip_pipe* p)
{
    size_t n = pipe_state_front_bytes(p, p->eng.hist_n, (int64_t)p->eng.pending(), (int64_t)p->demod_blocks.size());
    for (const Trailer& t : Trailers(p)) n += t.bytes(p);
    return n;
}

// What stands behind a trailing record's fixed part, between the state (at `host`) and the device.  The callers have waited for the first
// compute stream: a save comes behind the launches that wrote the device state, a restore behind the create call's memsets.
int trailer_copy(const sdrhip_pipe* p, const Trailer& t, unsigned char* host, hipMemcpyKind kind)
{
    const bool out = kind == hipMemcpyDeviceToHost;
    const size_t fb = (size_t)t.n_floats * sizeof(float);
    if (fb > 0) SDRHIP_CHECK_HIP(hipMemcpy(out ? (void*)host : t.floats, out ? (const void*)t.floats : host, fb, kind));
    return t.rows ? t.carry->host_copy(p->rows(), host + fb, t.rows[1], kind) : SDRHIP_OK;
}
}  // namespace

extern "C" {

size_t sdrhip_pipe_state_bytes(sdrhip_pipe* p)
{
    if (p == nullptr) return 0;
    // Exact, not an estimate: the pipe is drained here exactly as sdrhip_pipe_save will drain it (what is staged goes out, every
    // slot is harvested into the fifo), so the size returned is what the save that follows needs -- whatever the ratio of
    // the stage and the size of the blocks in flight.  0 = the drain failed (sdrhip_last_error).
    if (sdrhip_pipe_flush(p) < 0) return 0;
    return p->kind == PK_SPECTRUM ? spectrum_state_bytes(p) : pipe_state_size(p);
}

int sdrhip_pipe_save(sdrhip_pipe* p, void* buf, size_t capacity, size_t* used)
{
    SDRHIP_REQUIRE(p != nullptr && buf != nullptr && used != nullptr, "sdrhip_pipe_save");
    int rc = sdrhip_pipe_flush(p);
    if (rc < 0) return rc;
    const size_t need = p->kind == PK_SPECTRUM ? spectrum_state_bytes(p) : pipe_state_size(p);
    if (capacity < need) {
        set_error("sdrhip_pipe_save: %zu bytes needed, %zu given", need, capacity);
        return SDRHIP_ERR_ARG;
    }
    *used = need;
    if (p->kind == PK_SPECTRUM) return spectrum_save(p, buf);
    PipeStateHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kPipeMagic;
    h.version = pipe_state_version(p);
    h.kind = (int32_t)p->kind; h.block_out = p->block_out;
    h.I = p->I; h.D = p->D; h.Lp = p->Lp;
    h.cplx_in = p->cplx_in; h.cplx_out = p->cplx_out;
    h.uniform_n = p->uniform_n; h.all_uniform = p->all_uniform;
    h.n_blocks = (int32_t)p->demod_blocks.size();
    h.E_prev = p->E_prev; h.m_done = p->m_done; h.head_cap = p->eng.head_cap; h.hist_n = p->eng.hist_n; h.pending = (int64_t)p->eng.pending();
    h.last_re = p->last_re; h.last_im = p->last_im;
    SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));
    if (p->map_state.p) SDRHIP_CHECK_HIP(hipMemcpy(h.dc, p->map_state.p, sizeof h.dc, hipMemcpyDeviceToHost));
    memcpy(buf, &h, sizeof h);
    if (h.version == 2) {
        const PipeStateRows x = {p->rows(), (int32_t)p->fmt};
        memcpy((unsigned char*)buf + sizeof h, &x, sizeof x);
    }
    unsigned char* o = p->eng.save((unsigned char*)buf + pipe_state_header_bytes(p));
    for (int len : p->demod_blocks) { const int32_t v = len; memcpy(o, &v, sizeof v); o += sizeof v; }
    for (const Trailer& t : Trailers(p)) {
        memcpy(o, t.fixed, t.fixed_bytes);
        if ((rc = trailer_copy(p, t, o + t.fixed_bytes, hipMemcpyDeviceToHost)) != SDRHIP_OK) return rc;
        o += t.bytes(p);
    }
    return SDRHIP_OK;
}

int sdrhip_pipe_restore(sdrhip_pipe* p, const void* buf, size_t bytes)
{
    if (p != nullptr && p->kind == PK_SPECTRUM) return spectrum_restore(p, buf, bytes);
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
    if (p->kind == PK_DCBLOCK) {             // the two forms of the one-pole map kind: dc[2] holds alpha, 0 in a dcBlocker's state
        uint32_t theirs, mine;
        memcpy(&theirs, &h.dc[2], sizeof theirs);
        memcpy(&mine, &p->deemph_alpha, sizeof mine);
        SDRHIP_REQUIRE(theirs == 0 || mine != 0, "sdrhip_pipe_restore: the state belongs to a de-emphasis pipe, this is a dcBlocker pipe");
        SDRHIP_REQUIRE(theirs != 0 || mine == 0, "sdrhip_pipe_restore: the state belongs to a dcBlocker pipe, this is a de-emphasis pipe");
        SDRHIP_REQUIRE(theirs == mine, "sdrhip_pipe_restore: the state belongs to a de-emphasis pipe of another alpha");
    }
    SDRHIP_REQUIRE(h.hist_n >= 0 && h.hist_n <= h.head_cap && h.pending >= 0 && h.n_blocks >= 0 && h.E_prev >= h.hist_n && h.m_done >= 0,
                   "sdrhip_pipe_restore: inconsistent state");
    if (!p->is_map()) {
        // (the FIR-like stages and the banks)  the next pending output must start inside what the pipe has seen, every output
        // computable from those elements must be done at most once, and the history must reach back to its first input (3 elements of
        // alignment slack, 7 of u8, fir_submit): otherwise the kernels would be sent in front of the staging buffer
        const int64_t first_in = p->in_offset(h.m_done), m_max = p->outputs_by(h.E_prev), keep_from = p->keep_from(h.m_done, h.E_prev);
        SDRHIP_REQUIRE(h.m_done <= m_max && first_in <= h.E_prev + (p->Lp + p->D) / p->I + 1 && h.hist_n >= h.E_prev - keep_from,
                       "sdrhip_pipe_restore: the position and the history of the state do not belong together");
    }
    // Phase 1: every check, and room() (the one step that can fail for want of memory), before anything is put back, so that a refused
    // restore leaves the pipe fresh.  The fixed parts must all be there before any of them is read.
    const unsigned char* const front = (const unsigned char*)buf;
    Trailers trailers(p);
    size_t at = pipe_state_front_bytes(p, h.hist_n, h.pending, h.n_blocks), fixed = 0;
    for (const Trailer& t : trailers) fixed += t.rows ? t.fixed_bytes : t.bytes(p);
    SDRHIP_REQUIRE(bytes >= at + fixed, "sdrhip_pipe_restore: truncated state");
    int rc;
    for (Trailer& t : trailers) {
        if ((rc = t.check(p, front + at, h, t.fixed)) != SDRHIP_OK) return rc;
        const size_t y_n = t.rows ? (size_t)t.rows[1] : 0;
        SDRHIP_REQUIRE((bytes - at - t.fixed_bytes) / sizeof(float) >= (size_t)t.n_floats + (size_t)p->rows() * y_n * (t.rows ? t.carry->width : 1),
                       "sdrhip_pipe_restore: truncated state");
        at += t.bytes(p);
        if (t.rows && (rc = t.carry->room(p->rows(), t.rows[1] + 1, p->eng.compute[0])) != SDRHIP_OK) return rc;
    }
    // Phase 2: put it back.
    const unsigned char* in = p->eng.restore(front + pipe_state_header_bytes(p), h.hist_n, h.pending);
    p->E_prev = h.E_prev; p->m_done = h.m_done;
    p->uniform_n = h.uniform_n; p->all_uniform = h.all_uniform != 0;
    p->last_re = h.last_re; p->last_im = h.last_im;
    p->demod_blocks.clear();
    for (int i = 0; i < h.n_blocks; i++) { int32_t v; memcpy(&v, in, sizeof v); in += sizeof v; p->demod_blocks.push_back(v); }
    SDRHIP_CHECK_HIP(hipStreamSynchronize(p->eng.compute[0]));
    if (p->map_state.p) SDRHIP_CHECK_HIP(hipMemcpy(p->map_state.p, h.dc, sizeof h.dc, hipMemcpyHostToDevice));
    for (const Trailer& t : trailers) {
        if ((rc = trailer_copy(p, t, const_cast<unsigned char*>(in) + t.fixed_bytes, hipMemcpyHostToDevice)) != SDRHIP_OK) return rc;
        if (t.rows) { t.carry->a_done = t.rows[0]; t.carry->n = t.rows[1]; }
        in += t.bytes(p);
    }
    return ready_blocks(p);
}

}  // extern "C"
