// pipes_fir.cpp -- the FIR-like stages and the banks on host blocks: the push, the submission with its two bodies, the rows tail.
#include "pipe.hpp"

// ---- the rows tail: the stage behind a bank part, on the device rows (RowsCarry, pipe.hpp) --------------------------------------------
// Behind the bank part of a submission that wrote outputs [m_done, m_done + count) of every row behind the carried ones: the tail's
// outputs [a_done, a_end) into the chunk by ONE run (none when a_end == a_done), then the carry.  The narrow Pipe's run is the fused
// launch wherever it fits, whatever the bank's route setting and auto rule (those belong to sdrhip_narrow_bank_run).
// With an audio tail behind the narrow bank (narrow_audio) stage 2 writes behind the carried history of the second carry instead, ONE
// sdrhip_audio_tail_run_rows (route 0: the general fused kernel where its rule or mode 1 says so) computes the audio outputs
// [y2.a_done, q_end) into the chunk -- no tail launch when there is none -- and both carries step.
static int rows_tail(sdrhip_pipe* p, hipStream_t s, float* d_chunk, int64_t m_done, int64_t count, int64_t a_end, int64_t q_end)
{
    RowsCarry& y = p->y;
    const int K = p->rows();
    const int64_t n_y = y.n + count, y_base = m_done - y.n, n = a_end - y.a_done;
    if (n == 0) {
        y.n = n_y;
        return SDRHIP_OK;
    }
    int rc;
    float* d_out2 = d_chunk;
    int64_t stride2 = n;
    if (p->narrow_audio()) {
        if ((rc = p->y2.room(K, p->y2.n + n, s)) != SDRHIP_OK) return rc;
        d_out2 = p->y2.data() + p->y2.n;
        stride2 = p->y2.stride;
    }
    if (const NarrowBankDesc* nb = p->narrow) {
        const bool fm = nb->form == NARROW_FM, fused = narrow_stage2_fits(nb, K, y.data(), y.stride, y_base, y.a_done, a_end, p->block_mid);
        const size_t ws = narrow_stage2_bytes(nb, K, n, fused);
        if ((rc = grow(y.ws, ws > 16 ? ws : 16, s)) != SDRHIP_OK) return rc;
        if (fused && (rc = nb->d2->ensure_device()) != SDRHIP_OK) return rc;
        rc = narrow_stage2(nb, s, fused, y.data(), y.stride, y_base, n_y, d_out2, stride2, y.a_done, a_end, p->block_mid, fm ? p->fm.latest() : nullptr,
                           fm ? p->fm.out() : nullptr, nb->dc_block ? p->dc.out() : nullptr, (float*)y.ws.p, ws);
        if (rc == SDRHIP_OK && fm) p->fm.ran();
        if (rc == SDRHIP_OK && p->narrow_audio()) {
            RowsCarry& z = p->y2;
            const int64_t n_z = z.n + n, z_base = y.a_done - z.n, nq = q_end - z.a_done;
            if (nq == 0) {
                z.n = n_z;
            } else {
                const size_t wz = sdrhip_audio_tail_workspace_bytes(p->tail, K, n_z);
                if ((rc = grow(z.ws, wz, s)) != SDRHIP_OK) return rc;
                rc = sdrhip_audio_tail_run_rows(p->tail, s, z.data(), z.stride, z_base, n_z, d_chunk, nq, K, z.a_done, q_end, z.ws.p, wz);
                if (rc == SDRHIP_OK) rc = z.carry(K, n_z, a_end - sdrhip_audio_tail_first_input(p->tail, q_end), s);
            }
        }
    } else {
        const size_t ws = sdrhip_audio_tail_workspace_bytes(p->tail, K, n_y);
        if ((rc = grow(y.ws, ws, s)) != SDRHIP_OK) return rc;
        rc = sdrhip_audio_tail_run_rows(p->tail, s, y.data(), y.stride, y_base, n_y, d_chunk, n, K, y.a_done, a_end, y.ws.p, ws);
    }
    return rc != SDRHIP_OK ? rc : y.carry(K, n_y, m_done + count - p->tail_first_input(a_end), s);
}

// ---- one submission -------------------------------------------------------------------------------------------------------------------
// Where a submission stands in the stream: outputs [m_done, m_end) over input that starts at element in_base, the Cross outputs in
// front of m_split; uniform_seam as fir_submit's.  submit_parts: the launches of one submission, run(k_begin, k_end, seam_block,
// outputs in front of k_begin in this submission): a uniform run is ONE call over [m_done, m_end) with its seams; a ragged block is the
// Cross call over [m_done, m_split) (seam -1), then the One call over [m_split, m_end) (seam 0).  An empty part is no call.
struct Span {
    int64_t in_base, m_done, m_split, m_end, uniform_seam;
    int64_t tile_begin() const { return uniform_seam > 0 ? m_done : m_split; }      // the first output of the part that is not all Cross
    template <class Run>
    int submit_parts(Run run) const
    {
        const int64_t t0 = tile_begin();
        int r;
        if (t0 > m_done && (r = run(m_done, t0, (int64_t)-1, (int64_t)0)) != SDRHIP_OK) return r;
        return m_end > t0 ? run(t0, m_end, uniform_seam, t0 - m_done) : SDRHIP_OK;
    }
};

// filter / decimator / resampler, or the tuner's mix + decimator: in_base is the absolute stream position of din[0], which is what
// selects the oscillator phase
static int one_row_body(sdrhip_pipe* p, hipStream_t s, const float* din, float* dout, const Span& x)
{
    return x.submit_parts([&](int64_t k0, int64_t k1, int64_t seam, int64_t off) {
        float* o = dout + off * p->esz_out();
        if (p->kind == PK_RESAMPLER) return resamp_run(p->rs, s, din, x.in_base, o, k0, k1, seam, seam > 0 ? p->block_out : 0);
        if (p->kind == PK_TUNER) return tuner_run(p->tuner, s, din, IN_CF32, x.in_base, o, k0, k1, seam);
        return fir_run(p->fir, s, din, false, x.in_base, o, k0, k1, seam);
    });
}

// The banks: every row [cross | one] in the Pipe's form, row_len apart (dev_skew has aligned the tile part's first window).
// IQ: the bank's own rule picks the banked launch or channel by channel.  Envelopes and phases, one float per output: the
// fused launch (set) where it fits, else tuner bank + amDemod / fmDemod rows through the slot's complex scratch.
static int bank_body(sdrhip_pipe* p, hipStream_t s, int si, const void* d_in, float* dout, const Span& x, int64_t row_len, int64_t a_end,
                     int64_t q_end)
{
    const int K = p->rows();
    const int64_t count = x.m_end - x.m_done, np = row_floats(count);
    const int eo = p->narrow ? 2 : p->esz_out();      // floats per output of the bank part (the narrow Pipe's is complex, its chunk is not)
    int r;
    // where the form's rows end up: the result chunk, or (the rows tails) the device rows buffer behind the carried history
    float* fin = dout;
    int64_t fin_stride = row_len;
    if (p->rows_tail()) {
        if ((r = p->y.room(K, p->y.n + count, s)) != SDRHIP_OK) return r;
        fin = p->y.data() + p->y.n * p->y.width;
        fin_stride = p->y.stride;
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
    const int64_t t0 = x.tile_begin();
    float* iq = nullptr;
    if (p->pol.iq_always || (form.kind != BankForm::IQ && x.m_end > t0 &&
                             !bank_fused_fits(p->bank, bank_geom(p->fir, x.in_base, t0, x.m_end, x.uniform_seam), d_in, p->fmt, form, nullptr))) {
        if ((r = grow(p->iq_scratch[si], (size_t)K * 2 * (size_t)np * sizeof(float), s)) != SDRHIP_OK) return r;
        iq = (float*)p->iq_scratch[si].p;
    }
    r = x.submit_parts([&](int64_t k0, int64_t k1, int64_t seam, int64_t off) {
        float* o = out + off * eo;
        if (form.kind == BankForm::PHASE) {
            // each launch takes the state its predecessor left and leaves the next one's in the other array
            form.d_state = p->fm.latest();
            form.d_final = p->fm.out();
        }
        int rr;
        if (seam < 0) rr = bank_cross(p->bank, s, d_in, p->fmt, x.in_base, o, stride, k0, k1, form);
        else if (form.kind == BankForm::IQ) rr = tuner_bank_run(p->bank, s, d_in, p->fmt, x.in_base, o, stride, k0, k1, seam);
        else rr = bank_form_run(p->bank, s, d_in, p->fmt, x.in_base, o, stride, k0, k1, seam, form, iq);
        if (rr == SDRHIP_OK && form.kind == BankForm::PHASE) p->fm.ran();
        return rr;
    });
    if (r != SDRHIP_OK) return r;
    if (p->am_dc) {
        launch_dc_blocker_rows(s, K, count, out, np, fin, fin_stride, p->dc.latest(), p->dc.out(), out + (size_t)K * (size_t)np, 0);
        SDRHIP_CHECK_HIP(hipGetLastError());
    }
    return p->rows_tail() ? rows_tail(p, s, dout, x.m_done, count, a_end, q_end) : SDRHIP_OK;
}

// Submit the n elements staged in the current slot's pinned buffer.  uniform_seam > 0: they are whole blocks of that size
// and so was everything before them, so the seams of the reference's input buffers are the multiples of uniform_seam and
// ONE stream-API run covers the batch (interior seams included).  uniform_seam == 0: a single block of arbitrary size: the
// outputs straddling the boundary with the previous block first (all Cross), then the ones inside the new block (all One).
int fir_submit(sdrhip_pipe* p, int n, int64_t uniform_seam)
{
    HostStream& e = p->eng;
    const int si = e.cur();
    const size_t ein = p->ein();
    const int64_t E_prev = p->E_prev, E = E_prev + n;
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
    // staging buffer = [carried tail | staged elements]
    const int64_t keep_from = p->keep_from(p->m_done, E_prev);
    const Span x = {keep_from, p->m_done, m_split, p->outputs_by(E), uniform_seam};
    const int64_t tail = E_prev - keep_from;
    const uint8_t* first = e.carry(keep_from, E_prev, n, "pipe");
    if (first == nullptr) return SDRHIP_ERR_STATE;
    const bool direct = p->direct_ok && (size_t)(tail + n) * ein <= sdrhip_pipe::kDirectBytes;
    // in-place pushes go to their slot's own compute stream: nothing push i+1 computes depends on what push i left on the
    // device (the carried tail comes from the host-side history), so consecutive pushes overlap on the GPU -- unless the pipe keeps
    // state on the device from submission to submission (PipePolicy::stream0)
    hipStream_t cs = direct && !p->pol.stream0 ? e.compute[si] : e.compute[0];
    // a submission that is not read in place is, up to the direct bound, ONE copy into device memory on the slot's own stream and the
    // launch behind it
    const HostStream::Route route = !direct ? HostStream::kCopyEngines : p->pol.in_place ? HostStream::kInPlace : HostStream::kSlotStream;
    if (p->pol.align_first && route != HostStream::kInPlace) {
        // the copy may land anywhere in the slot's device buffer: put the banked launch's first window on a 16-byte boundary there,
        // which the staging buffer cannot promise once a block had an odd size
        const size_t off = (size_t)(x.tile_begin() * p->D - keep_from) * ein;
        e.dev_skew = (16 - off % 16) % 16;
    }
    // the rows tails: the chunk holds the tail's outputs that became ready, [a_done, a_end) of every row
    const bool tailed = p->rows_tail();
    int64_t a_end = p->y.a_done;
    if (tailed) a_end = std::max(a_end, p->tail_ready(x.m_end));
    int64_t q_end = p->y2.a_done;                 // (narrow_audio: the audio outputs the stage-2 outputs so far complete)
    const int64_t row_len = tailed ? p->chunk_outputs(a_end, &q_end) : (x.m_end - x.m_done) * p->esz_out();
    int rc = e.submit(route, cs, first, (size_t)(tail + n) * ein, p->rows() * row_len, [&](hipStream_t s, const void* d_in, void* d_out) {
        if (p->bank == nullptr) return one_row_body(p, s, (const float*)d_in, (float*)d_out, x);
        return bank_body(p, s, si, d_in, (float*)d_out, x, row_len, a_end, q_end);
    }, tailed && x.m_end > x.m_done);
    if (rc != SDRHIP_OK) return rc;
    p->m_done = x.m_end;
    p->E_prev = E;
    p->y.a_done = a_end;
    p->y2.a_done = q_end;
    return SDRHIP_OK;
}

// the reference's `assert "filter 1" / "decimate 1" / "resample 1"` for a block of n elements arriving at E_at: after the
// crossover the rest of the new buffer must still hold one whole filter
static int fir_check_block(const sdrhip_pipe* p, int64_t E_at, int64_t m_pending, int n)
{
    int64_t m_split = ceil_div64(E_at * p->I, p->D);
    if (m_split < m_pending) m_split = m_pending;
    if (p->outputs_by(E_at + n) <= m_split) {
        set_error("pipe: input block of %d elements is shorter than the filter (numCoeffs %d): the reference asserts "
                  "(Filter.hs:544,586,691)", n, p->Lp);
        return SDRHIP_ERR_ARG;
    }
    return SDRHIP_OK;
}

int fir_like_push(sdrhip_pipe* p, const void* block, int n)
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
    const int64_t m_pending = e.staged > 0 ? p->outputs_by(p->E_prev + e.staged) : p->m_done;
    if ((rc = fir_check_block(p, p->E_prev + e.staged, m_pending, n)) != SDRHIP_OK) return rc;
    p->uniform_n = uni;
    p->all_uniform = all_uniform;
    const int64_t cap = coalescing ? (int64_t)ce * p->uniform_n : n;
    if ((rc = p->open_slot((size_t)(cap > e.staged + n ? cap : e.staged + n))) != SDRHIP_OK) return rc;
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
