// pipes_spectrum.cpp -- the waterfall Pipe (sdrhip_pipe_spectrum), the spectrum operator's reducing form on the host-block engine.
// With S the samples pushed so far, output row R exists once (R group + group - 1) hop + n <= |S| and is row R of ONE
// sdrhip_spectrum_reduce_run_device over S.  The host keeps the samples from row sp.rows_done's first one onward: the engine's history
// while no row is complete, [history | staged] in the slot's staging buffer once one is (a submission, or rows piling up behind a
// busy GPU / a coalesce count).  A submission is one reduce run over [tail | staged] with rows_out = every complete row.
#include "pipe.hpp"

static constexpr size_t kSpectrumTailBytes = 4 << 20;     // the engine's adaptive staging cap: the bound of the carried tail

static int64_t spectrum_rows_in(const sdrhip_pipe* p, int64_t avail)
{
    if (avail < p->block_out) return 0;
    return ((avail - p->block_out) / p->sp.hop + 1) / p->sp.group;
}

static int spectrum_submit(sdrhip_pipe* p)
{
    HostStream& e = p->eng;
    const SpectrumPart& sp = p->sp;
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
    const bool scratch = spectrum_reduce_uses_scratch(sp.spec, sp.group);
    hipStream_t cs = direct && !scratch ? e.compute[si] : e.compute[0];
    const int n = p->block_out;
    int rc = e.submit(direct ? HostStream::kSlotStream : HostStream::kCopyEngines, cs, first, (size_t)have * ein, r * n,
                      [&](hipStream_t s, const void* d_in, void* d_out) {
        return sdrhip_spectrum_reduce_run_device(sp.spec, s, d_in, have, sp.hop, (int)r, sp.group, sp.reduce, sp.unit, sp.floor_db, (float*)d_out);
    });
    if (rc != SDRHIP_OK) return rc;
    // the next tail starts at stream sample (rows_done + r) group hop: inside [tail | staged] (still in the slot's staging buffer, which
    // nothing writes before the slot is reopened), or `skip` samples beyond its end
    const int64_t used = r * sp.group * sp.hop;
    if (used < have) {
        e.hist_n = have - used;
        memcpy(e.hist.data(), first + (size_t)used * ein, (size_t)e.hist_n * ein);
    } else {
        e.hist_n = 0;
        p->sp.skip = used - have;
    }
    p->sp.rows_done += r;
    return SDRHIP_OK;
}

// room for `elems` staged elements in the current slot; growth doubles, so that small pushes piling up do not re-pin every time
int spectrum_open_slot(sdrhip_pipe* p, int64_t elems)
{
    HostStream& e = p->eng;
    const size_t ein = p->ein(), head = (size_t)e.head_cap * ein, cap = e.slot[e.cur()].hin.cap;
    size_t bytes = (size_t)elems * ein;
    if (cap < head + bytes && cap > head && bytes < 2 * (cap - head)) bytes = 2 * (cap - head);
    return e.open_slot(bytes, (size_t)(e.staged + p->lent) * ein);
}

int spectrum_push(sdrhip_pipe* p, const void* block, int n)
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
    const int64_t drop = p->sp.skip < n ? p->sp.skip : n;
    const int m = n - (int)drop;
    p->sp.skip -= drop;
    p->sp.pos += n;
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
int spectrum_settle(sdrhip_pipe* p)
{
    p->lent = 0;
    return p->eng.staged > 0 ? spectrum_submit(p) : SDRHIP_OK;
}

extern "C" int sdrhip_pipe_spectrum(sdrhip_pipe** pp, sdrhip_spectrum* s, int64_t hop, int group, int reduce, int unit, double floor_db)
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
    int rc = pipe_new(pp, PK_SPECTRUM, nullptr, nullptr, n, true, false, 1, 1, 1, fmt, max_tail > 0 ? max_tail : 1);
    if (rc != SDRHIP_OK) return rc;
    SpectrumPart& sp = (*pp)->sp;
    sp.spec = s;
    sp.hop = hop; sp.group = group; sp.reduce = reduce; sp.unit = unit; sp.floor_db = floor_db;
    return SDRHIP_OK;
}

// ---- the saved state, version 3 -------------------------------------------------------------------------------------------------------
// This header, the carried tail (tail_n samples in the input's own type), the rows not yet popped (pending floats).  pos = samples
// pushed so far; the tail starts at stream sample rows_done * group * hop = pos - tail_n (skip == 0) or lies skip samples beyond pos
// (tail_n == 0).
namespace {
struct PipeStateSpectrum {
    uint32_t magic, version;
    int32_t kind, n, input_type, group, reduce, unit;
    int64_t hop;
    double floor_db;
    int64_t pos, rows_done, skip, tail_n, pending;
};
constexpr uint32_t kPipeSpectrumVersion = 3;
}  // namespace

size_t spectrum_state_bytes(const sdrhip_pipe* p)
{
    return sizeof(PipeStateSpectrum) + p->eng.state_bytes(p->eng.hist_n, (int64_t)p->eng.pending());
}

int spectrum_save(sdrhip_pipe* p, void* buf)        // (behind sdrhip_pipe_save's flush and capacity check)
{
    const SpectrumPart& sp = p->sp;
    PipeStateSpectrum x;
    memset(&x, 0, sizeof x);
    x.magic = kPipeMagic; x.version = kPipeSpectrumVersion; x.kind = (int32_t)p->kind;
    x.n = p->block_out; x.input_type = (int32_t)p->fmt; x.group = sp.group; x.reduce = sp.reduce; x.unit = sp.unit;
    x.hop = sp.hop; x.floor_db = sp.floor_db;
    x.pos = sp.pos; x.rows_done = sp.rows_done; x.skip = sp.skip; x.tail_n = p->eng.hist_n; x.pending = (int64_t)p->eng.pending();
    memcpy(buf, &x, sizeof x);
    (void)p->eng.save((unsigned char*)buf + sizeof x);
    return SDRHIP_OK;
}

int spectrum_restore(sdrhip_pipe* p, const void* buf, size_t bytes)
{
    SpectrumPart& sp = p->sp;
    SDRHIP_REQUIRE(buf != nullptr && bytes >= 3 * sizeof(int32_t), "sdrhip_pipe_restore");
    SDRHIP_REQUIRE(p->eng.pushes == 0 && p->sp.pos == 0 && p->eng.staged == 0 && p->eng.pending() == 0,
                   "sdrhip_pipe_restore: only into a pipe that has not been pushed to");
    PipeStateSpectrum x;
    memset(&x, 0, sizeof x);
    memcpy(&x, buf, bytes < sizeof x ? bytes : sizeof x);
    SDRHIP_REQUIRE(x.magic == kPipeMagic, "sdrhip_pipe_restore: not a pipe state");
    SDRHIP_REQUIRE(x.version == kPipeSpectrumVersion && x.kind == (int32_t)PK_SPECTRUM, "sdrhip_pipe_restore: the state belongs to a pipe of another kind");
    SDRHIP_REQUIRE(bytes >= sizeof x, "sdrhip_pipe_restore: truncated state");
    SDRHIP_REQUIRE(x.n == p->block_out && x.input_type == (int32_t)p->fmt && x.hop == sp.hop && x.group == sp.group && x.reduce == sp.reduce &&
                       x.unit == sp.unit && memcmp(&x.floor_db, &sp.floor_db, sizeof(double)) == 0,
                   "sdrhip_pipe_restore: the state belongs to a waterfall pipe of other parameters");
    // the tail holds no whole row and starts where row rows_done does
    const __int128 start = (__int128)x.rows_done * sp.group * sp.hop;
    SDRHIP_REQUIRE(x.pos >= 0 && x.rows_done >= 0 && x.skip >= 0 && x.tail_n >= 0 && x.pending >= 0 && x.pending % p->block_out == 0 &&
                       x.tail_n <= p->eng.head_cap && (x.skip == 0 || x.tail_n == 0) && start == (__int128)x.pos - x.tail_n + x.skip &&
                       spectrum_rows_in(p, x.tail_n) == 0,
                   "sdrhip_pipe_restore: inconsistent state");
    SDRHIP_REQUIRE(x.pending <= (int64_t)((bytes - sizeof x) / sizeof(float)) &&
                       bytes - sizeof x >= p->eng.state_bytes(x.tail_n, x.pending), "sdrhip_pipe_restore: truncated state");
    (void)p->eng.restore((const unsigned char*)buf + sizeof x, x.tail_n, x.pending);
    sp.pos = x.pos; sp.rows_done = x.rows_done; sp.skip = x.skip;
    return ready_blocks(p);
}
