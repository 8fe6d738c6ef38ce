// host_stream.hpp -- the submission engine of the host-block operators: sdrhip_fm_stream_* (chain.cpp) and the Pipes
// (sdrhip_pipe_*, pipes.cpp).  What the kernels compute stays with the operator; this is how host blocks reach them and how the
// results come back.
//
// The pinned staging buffer of a slot holds [carried tail | staged elements] contiguously: the tail (the elements earlier pushes
// delivered and pending outputs still need) is kept in a small host-side history and copied in front of the staged elements by
// the host, so the device never shuffles it.  A submission then takes one of three routes, chosen by the operator:
//   * kInPlace: the kernels read the pinned staging buffer and write the pinned result buffer over PCIe -- no copy, one event;
//   * kSlotStream: ONE H2D copy into device memory on the compute stream, the kernels on device memory, the results written to
//     pinned memory -- the copy and the kernels are ordered by their stream, one event;
//   * kCopyEngines: H2D on the upload stream, the kernels on the compute stream after its event, D2H on the download stream
//     after theirs -- the upload of submission i overlaps the compute of i-1 and the download of i-2.
// Up to nslots submissions are in flight, so results lag at most nslots - 1 submissions (flush drains); their output floats go
// into a fifo in submission order.
//
// Rows (sdrhip_fm_stream over a receiver bank): an operator of `rows` > 1 outputs writes, per submission, `rows` rows of
// out_floats / rows floats each into the result buffer, row after row.  Chunk sizes differ from submission to submission, so the
// harvest regroups them: one fifo per row, each in submission order, all of the same length and read by ONE cursor.  rows == 1
// (every Pipe, a chain's stream) is the single fifo it always was.
#pragma once
#include <string.h>

#include <optional>
#include <utility>
#include <vector>

#include "common.hpp"

namespace sdrhip {

// The environment knobs of the host-block operators, read once per process.
struct StreamKnobs {
    bool direct = true;                          // SDRHIP_NO_DIRECT_STREAM unset: small submissions may run in place
    int slots = 0;                               // SDRHIP_STREAM_SLOTS=2..4: submissions in flight (0: the operator's default)
    std::optional<int64_t> adaptive;             // SDRHIP_STREAM_ADAPTIVE: cap of the default adaptive submission, source blocks
    std::optional<int64_t> adaptive_bytes;       // SDRHIP_ADAPTIVE_BYTES: what a Pipe's adaptive submission stages at most
};

inline const StreamKnobs& stream_knobs()
{
    static const StreamKnobs k = [] {
        StreamKnobs s;
        s.direct = getenv("SDRHIP_NO_DIRECT_STREAM") == nullptr;
        if (const char* e = getenv("SDRHIP_STREAM_SLOTS"))
            if (atoi(e) >= 2 && atoi(e) <= 4) s.slots = atoi(e);
        if (const char* e = getenv("SDRHIP_STREAM_ADAPTIVE")) s.adaptive = atoll(e);
        if (const char* e = getenv("SDRHIP_ADAPTIVE_BYTES")) s.adaptive_bytes = atoll(e);
        return s;
    }();
    return k;
}

struct HostStream {
    static constexpr int kMaxSlots = 4;
    enum Route { kInPlace, kSlotStream, kCopyEngines };
    struct Slot {
        PinBuf hin, hout;               // staging buffer [carried tail | staged elements]; results
        DevBuf din, dout;               // device input / output of the copy routes
        hipEvent_t ev = nullptr;        // results in hout (in place: the staging buffer is free again too)
        hipEvent_t ev_up = nullptr;     // H2D complete (kCopyEngines)
        hipEvent_t ev_k = nullptr;      // kernels complete (kCopyEngines)
        int64_t n_out = 0;              // floats produced by the in-flight submission
        bool busy = false;
        bool direct = false;            // the last submission did not use the upload stream: `ev` also releases the staging buffer
    } slot[kMaxSlots];
    int nslots = 2;
    hipStream_t compute[kMaxSlots] = {nullptr, nullptr, nullptr, nullptr};   // the slots' compute streams; [0] also the copy route's
    hipStream_t up = nullptr, down = nullptr;
    int64_t pushes = 0;             // submissions so far (slot = pushes % nslots)
    int staged = 0;                 // elements staged in the current slot, not yet submitted
    size_t esz = 1;                 // bytes per element
    int64_t head_cap = 0;           // elements of room in front of the staged ones for the carried tail
    std::vector<uint8_t> hist;      // the stream's last hist_n elements (host copy)
    int64_t hist_n = 0;
    std::vector<float> fifo;        // produced floats not yet popped: contiguous storage + read cursor (row 0)
    size_t head = 0;
    int rows = 1;                   // outputs per operator (set before the first submission)
    // Bytes (< 64) the copy routes leave in front of the NEXT submission in the slot's device buffer: the operator's way to put a
    // window it cares about on a 16-byte boundary there whatever the carried tail's length is.  Back to 0 after every submission.
    size_t dev_skew = 0;
    std::vector<std::vector<float>> more;    // rows 1 .. rows - 1: as long as `fifo`, read by the same cursor
    std::vector<float>& row(int r) { return r == 0 ? fifo : more[(size_t)r - 1]; }
    const std::vector<float>& row(int r) const { return r == 0 ? fifo : more[(size_t)r - 1]; }
    void set_rows(int n)
    {
        rows = n;
        more.assign((size_t)n - 1, std::vector<float>());
    }

    // nslots = SDRHIP_STREAM_SLOTS, else default_slots; `who` prefixes the error message
    int init(int default_slots, size_t elem_bytes, int64_t head_room, const char* who)
    {
        nslots = stream_knobs().slots ? stream_knobs().slots : default_slots;
        esz = elem_bytes;
        head_cap = head_room;
        hist.assign((size_t)head_cap * esz, 0);
        hipError_t e = hipSuccess;
        for (int i = 0; i < nslots; i++)
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&compute[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&down, hipStreamNonBlocking);
        for (auto& sl : slot)
            for (hipEvent_t* ev : {&sl.ev, &sl.ev_up, &sl.ev_k})
                if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            set_error("%s: %s", who, hipGetErrorString(e));
            return SDRHIP_ERR_HIP;
        }
        return SDRHIP_OK;
    }
    ~HostStream()
    {
        for (hipStream_t st : {up, compute[0], compute[1], compute[2], compute[3], down})
            if (st) (void)hipStreamSynchronize(st);
        for (auto& sl : slot)
            for (hipEvent_t e : {sl.ev, sl.ev_up, sl.ev_k})
                if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : {up, compute[0], compute[1], compute[2], compute[3], down})
            if (st) (void)hipStreamDestroy(st);
    }
    int sync()
    {
        for (hipStream_t st : {up, compute[0], compute[1], compute[2], compute[3], down})
            if (st) SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
        return SDRHIP_OK;
    }

    int cur() const { return (int)(pushes % nslots); }
    uint8_t* staged_base() const { return (uint8_t*)slot[cur()].hin.p + (size_t)head_cap * esz; }   // staged element 0
    uint8_t* write_pos() const { return staged_base() + (size_t)staged * esz; }
    // is the slot the next submission moves on to still running on the GPU?
    bool next_in_flight() const
    {
        const Slot& sl = slot[(cur() + 1) % nslots];
        return sl.busy && hipEventQuery(sl.ev) == hipErrorNotReady;
    }
    size_t pending() const { return fifo.size() - head; }     // floats PER ROW
    void take(size_t nfloats, float* out)
    {
        memcpy(out, fifo.data() + head, nfloats * sizeof(float));
        head += nfloats;
    }
    // the next nfloats of every row: row r's to out + r * stride
    void take_rows(size_t nfloats, float* out, int64_t stride)
    {
        for (int r = 0; r < rows; r++) memcpy(out + (int64_t)r * stride, row(r).data() + head, nfloats * sizeof(float));
        head += nfloats;
    }

    int harvest(int si)
    {
        Slot& sl = slot[si];
        if (!sl.busy) return SDRHIP_OK;
        SDRHIP_CHECK_HIP(hipEventSynchronize(sl.ev));
        const size_t old_head = head, per_row = (size_t)sl.n_out / (size_t)rows;
        for (int r = 0; r < rows; r++) {
            std::vector<float>& f = row(r);
            head = old_head;                                     // one cursor: every row is compacted the same way
            if (head > 0 && head == f.size()) { f.clear(); head = 0; }
            else if (head > (1u << 20) && head * 2 > f.size()) { f.erase(f.begin(), f.begin() + head); head = 0; }   // compact occasionally
            const size_t old = f.size();
            f.resize(old + per_row);
            if (per_row > 0) memcpy(f.data() + old, (const float*)sl.hout.p + (size_t)r * per_row, per_row * sizeof(float));
        }
        sl.busy = false;
        return SDRHIP_OK;
    }
    // harvest, oldest first, every in-flight submission the GPU has finished (never waits)
    int harvest_done()
    {
        for (int64_t k = pushes - (nslots - 1); k < pushes; k++) {
            if (k < 0) continue;
            const int si = (int)(k % nslots);
            if (!slot[si].busy) continue;
            if (hipEventQuery(slot[si].ev) != hipSuccess) break;     // still running (an error surfaces in the blocking harvest)
            int rc = harvest(si);
            if (rc != SDRHIP_OK) return rc;
        }
        return SDRHIP_OK;
    }
    // harvest every slot, oldest first: the results go into the fifo in submission order
    int flush()
    {
        const int first = cur();
        for (int k = 0; k < nslots; k++) {
            int rc = harvest((first + k) % nslots);
            if (rc != SDRHIP_OK) return rc;
        }
        return SDRHIP_OK;
    }

    // Make the current slot's staging buffer writable and `bytes` long behind the head room.  When nothing is staged yet, the
    // slot's previous submission is harvested and its upload / in-place read must have left the buffer: growing frees it.
    // (A busy slot's harvest has waited for `ev`, the last event of every route; a submission without outputs left only the
    // upload or in-place event to wait for.)  Growing keeps the first `keep` bytes behind the head room: what is staged, and
    // what the caller was lent behind it (a block handed out for an in-place push and not pushed yet).
    int open_slot(size_t bytes, size_t keep)
    {
        Slot& sl = slot[cur()];
        int rc;
        if (staged == 0) {
            const bool waited = sl.busy;
            if ((rc = harvest(cur())) != SDRHIP_OK) return rc;
            if (!waited) SDRHIP_CHECK_HIP(hipEventSynchronize(sl.direct ? sl.ev : sl.ev_up));
        }
        const size_t head_bytes = (size_t)head_cap * esz;
        if (sl.hin.cap < head_bytes + bytes) {
            PinBuf bigger;
            if ((rc = bigger.ensure(head_bytes + bytes)) != SDRHIP_OK) return rc;
            if (sl.hin.cap < head_bytes) keep = 0;
            else if (keep > sl.hin.cap - head_bytes) keep = sl.hin.cap - head_bytes;
            if (keep > 0) memcpy((char*)bigger.p + head_bytes, (char*)sl.hin.p + head_bytes, keep);
            std::swap(sl.hin.p, bigger.p);
            std::swap(sl.hin.cap, bigger.cap);
            std::swap(sl.hin.dev, bigger.dev);
        }
        return SDRHIP_OK;
    }

    // Put the carried tail -- the history's elements [keep_from, end) of the stream -- in front of the n staged elements and keep
    // the last head_cap elements of [tail | staged] as the next history (the tail alone may not reach back far enough, the staged
    // elements alone may be fewer than head_cap).  Returns the tail's first element; nullptr (SDRHIP_ERR_STATE) when the history
    // or the head room does not cover the tail: a state that says so came from a corrupt or hand-built checkpoint, and running on
    // would index in front of the staging buffer.
    uint8_t* carry(int64_t keep_from, int64_t end, int64_t n, const char* who)
    {
        const int64_t tail = end - keep_from;
        if (tail > hist_n) {
            set_error("%s: the history holds %lld elements but the carried tail needs %lld", who, (long long)hist_n, (long long)tail);
            return nullptr;
        }
        if (tail > head_cap) {
            set_error("%s: carried tail of %lld elements exceeds the head room (%lld)", who, (long long)tail, (long long)head_cap);
            return nullptr;
        }
        uint8_t* first = staged_base() - (size_t)tail * esz;
        if (tail > 0) memcpy(first, hist.data() + (size_t)(hist_n - tail) * esz, (size_t)tail * esz);
        const int64_t have = tail + n;
        const int64_t keep = have < head_cap ? have : head_cap;
        memmove(hist.data(), first + (size_t)(have - keep) * esz, (size_t)keep * esz);
        hist_n = keep;
        return first;
    }

    // Submit the current slot: `first` .. `first + in_bytes` is its [carried tail | staged] in the staging buffer, out_floats
    // results are expected (none: no launch; with rows > 1 the total of all rows, each out_floats / rows long).  launch(stream, d_in, d_out) enqueues the operator's kernels on `stream` and
    // returns an SDRHIP_* code.  The oldest submission is harvested afterwards: its slot is the next to be filled.
    // always_launch: the operator keeps state on the device that every submission moves on (the audio Pipes' demodulated rows), so
    // launch() runs even when no result is expected -- with d_out as it happens to be (possibly null) -- and the slot counts as busy
    // with no floats to harvest, so that its buffers are not reused before those kernels are done.
    template <class Launch>
    int submit(Route route, hipStream_t cs, const void* first, size_t in_bytes, int64_t out_floats, Launch&& launch, bool always_launch = false)
    {
        const bool run = out_floats > 0 || always_launch;
        Slot& sl = slot[cur()];
        const size_t out_bytes = (size_t)out_floats * sizeof(float);
        int rc;
        sl.n_out = 0;
        if (out_floats > 0 && (rc = sl.hout.ensure(out_bytes)) != SDRHIP_OK) return rc;
        if (route != kCopyEngines) {
            if (run) {
                const void* d_in = sl.hin.dev_ptr(first);
                if (route == kSlotStream) {
                    if ((rc = sl.din.ensure(in_bytes + 64 + dev_skew)) != SDRHIP_OK) return rc;
                    SDRHIP_CHECK_HIP(hipMemcpyAsync((char*)sl.din.p + dev_skew, first, in_bytes, hipMemcpyHostToDevice, cs));
                    d_in = (const char*)sl.din.p + dev_skew;
                }
                if ((rc = launch(cs, d_in, sl.hout.dev)) != SDRHIP_OK) return rc;
                sl.n_out = out_floats;
                sl.busy = true;
            }
            // ONE event per submission: the results are in pinned memory and the staging buffer is free again when the kernels are done
            SDRHIP_CHECK_HIP(hipEventRecord(sl.ev, cs));
            sl.direct = true;
        } else {
            // the slot's device buffer was last read by submission i - nslots, harvested before the slot was reopened
            if ((rc = sl.din.ensure(in_bytes + 64 + dev_skew)) != SDRHIP_OK) return rc;
            SDRHIP_CHECK_HIP(hipMemcpyAsync((char*)sl.din.p + dev_skew, first, in_bytes, hipMemcpyHostToDevice, up));
            SDRHIP_CHECK_HIP(hipEventRecord(sl.ev_up, up));
            sl.direct = false;
            if (run && out_floats == 0) {
                SDRHIP_CHECK_HIP(hipStreamWaitEvent(cs, sl.ev_up, 0));
                if ((rc = launch(cs, (const void*)((const char*)sl.din.p + dev_skew), sl.dout.p)) != SDRHIP_OK) return rc;
                SDRHIP_CHECK_HIP(hipEventRecord(sl.ev, cs));
                sl.busy = true;
            }
            if (out_floats > 0) {
                SDRHIP_CHECK_HIP(hipStreamWaitEvent(cs, sl.ev_up, 0));
                if ((rc = sl.dout.ensure(out_bytes)) != SDRHIP_OK) return rc;
                if ((rc = launch(cs, (const void*)((const char*)sl.din.p + dev_skew), sl.dout.p)) != SDRHIP_OK) return rc;
                SDRHIP_CHECK_HIP(hipEventRecord(sl.ev_k, cs));
                SDRHIP_CHECK_HIP(hipStreamWaitEvent(down, sl.ev_k, 0));
                SDRHIP_CHECK_HIP(hipMemcpyAsync(sl.hout.p, sl.dout.p, out_bytes, hipMemcpyDeviceToHost, down));
                SDRHIP_CHECK_HIP(hipEventRecord(sl.ev, down));
                sl.n_out = out_floats;
                sl.busy = true;
            }
        }
        pushes++;
        staged = 0;
        dev_skew = 0;
        return harvest(cur());
    }

    // ---- checkpoint / resume: the history (hist_n elements) and the fifo (floats not yet popped; n_pending of them PER ROW, row
    // after row), in this order, behind the operator's own header
    size_t state_bytes(int64_t n_hist, int64_t n_pending) const
    {
        return (size_t)n_hist * esz + (size_t)rows * (size_t)n_pending * sizeof(float);
    }
    unsigned char* save(unsigned char* o) const
    {
        if (hist_n > 0) memcpy(o, hist.data(), (size_t)hist_n * esz);
        o += (size_t)hist_n * esz;
        for (int r = 0; r < rows; r++) {
            if (pending() > 0) memcpy(o, row(r).data() + head, pending() * sizeof(float));
            o += pending() * sizeof(float);
        }
        return o;
    }
    const unsigned char* restore(const unsigned char* in, int64_t n_hist, int64_t n_pending)
    {
        const size_t hist_bytes = (size_t)n_hist * esz;
        if (hist.size() < hist_bytes) hist.resize(hist_bytes);
        if (hist_bytes) memcpy(hist.data(), in, hist_bytes);
        in += hist_bytes;
        hist_n = n_hist;
        head = 0;
        for (int r = 0; r < rows; r++) {
            row(r).resize((size_t)n_pending);    // (memcpy: the floats need not be aligned inside the caller's buffer)
            if (n_pending > 0) memcpy(row(r).data(), in, (size_t)n_pending * sizeof(float));
            in += (size_t)n_pending * sizeof(float);
        }
        return in;
    }
};

}  // namespace sdrhip
