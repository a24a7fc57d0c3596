// encoder.h -- host control plane of the encoder.
//
// Decision logic (window bookkeeping, path selection, row numbering, footer)
// follows the reference encoder exactly so the emitted bit stream is
// identical (reference SiameseEncoder.h:104-421, SiameseEncoder.cpp:56-1441).
// Every symbol-sized operation is emitted as a device op into this
// instance's Program; the symbols themselves live in HBM.
#pragma once

#include "arq.h"
#include "codedef.h"
#include "engine.h"
#include "objpool.h"
#include "../../include/siamese.h"

#include <memory>
#include <vector>

namespace sgpu {

struct EncSlot
{
    DevBuf buf;                 // [length prefix || payload] in HBM
    bool inSlab = false;        // buf is a slot of the subwindow's slab (not owned)
    unsigned bytes = 0;         // prefix + payload
    unsigned column = 0;
    unsigned header = 0;        // length-prefix bytes
    uint32_t lastSend = 0;      // msec timestamp of the last (re)send (ARQ)
    // host mirror (drop-in mode only): out of line, so the batch path's
    // window scans touch a 48-byte slot
    std::unique_ptr<std::vector<uint8_t>> hostp;
    std::vector<uint8_t>& host()
    {
        if (!hostp)
            hostp.reset(new std::vector<uint8_t>);
        return *hostp;
    }
};

/// A subwindow whose originals came from range adds of one length says in one
/// descriptor what its slot records would say, and leaves them unwritten
/// ("uniform").  Slot i of `mask` has buf = {slab.buf.ptr + i * slab.stride,
/// slab.stride}, inSlab, the shared bytes and header, column first + i and
/// lastSend = stamp.  Slots outside the mask are fresh.
struct EncUniform
{
    uint64_t mask = 0;          // slots described (0: the subwindow is not uniform)
    unsigned bytes = 0;         // prefix + payload of each
    unsigned header = 0;
    unsigned first = 0;         // column of slot 0
    uint32_t stamp = 0;         // lastSend of each
};

struct EncSubwindow
{
    EncSlot slot[kSubwindow];
    Slab slab;                  // the slots' shared buffer (engine.h)
    // every slot in its fresh state: from the pool until a slot record is
    // written (EncoderCore::slot, place), and again after the owner's teardown
    bool clean = false;
    EncUniform uni;
#ifdef SGPU_SLOT_CHECK
    // (the test double's build) the records the per-element code would have
    // written for the uniform slots, compared with the descriptor's view
    EncSlot shadow[kSubwindow];
#endif
};

/// unique_ptr deleter: subwindows go back to the thread's pool, emptied
/// (their buffers were released by the owner).
struct EncSubwindowRecycle
{
    void operator()(EncSubwindow* w) const
    {
        w->uni = EncUniform();
        if (!w->clean) {
            w->slab = Slab();
            for (EncSlot& s : w->slot) {
                s.buf = DevBuf();
                s.inSlab = false;
                s.bytes = s.column = s.header = 0;
                s.lastSend = 0;
                if (s.hostp)
                    s.hostp->clear();
            }
            w->clean = true;
        }
        ObjPool<EncSubwindow>::put(w);
    }
};
using EncSubwindowPtr = std::unique_ptr<EncSubwindow, EncSubwindowRecycle>;

/// Running sum of one (lane, sum-index) in HBM.
struct DevSum
{
    DevBuf buf;
    unsigned bytes = 0;     // logical length (reference Buffer.Bytes)
    unsigned devValid = 0;  // bytes actually materialised on the device
};

/// Result of an encode in device terms.
struct EncodeOut
{
    DevBuf buf;             // recovery packet (valid until the next encode)
    unsigned bytes = 0;     // payload + footer
    uint8_t footer[kMaxFooterBytes] = {};
    unsigned footerBytes = 0;
    uint8_t head[kMaxLengthPrefix] = {}; // first bytes (single-packet rows only)
    RowMeta meta;
};

class EncoderCore
{
public:
    EncoderCore(Engine* eng, bool hostMirror);
    ~EncoderCore();

    Program& program() { return prog_; }

    unsigned remaining_slots() const { return kMaxPacketsInFlight - count_; }

    /// siamese_encoder_add.  Source is host memory or (device != 0) HBM.
    SiameseResult add(SiameseOriginalPacket& packet, uint64_t deviceSrc = 0);
    /// `count` adds of device originals in one call (sgpu_encoder_add_range):
    /// original k at src + k * srcStride, lens[k] bytes (fixedBytes when lens
    /// is null).  Identical to `count` add() calls that stop at the first
    /// failure, whose result is returned; *added originals were taken, the
    /// first as packet *firstNum (the rest follow it).  Consecutive slab slots
    /// become one ingest run.
    SiameseResult add_range(uint64_t src, uint32_t srcStride, const unsigned* lens, unsigned fixedBytes,
                            unsigned count, unsigned* firstNum, unsigned* added);
    void remove_before(unsigned firstKeptColumn);
    SiameseResult get(SiameseOriginalPacket& packet);
    /// sgpu_encoder_deliver_range: queue the framing of originals firstNum,
    /// firstNum + 1, ... into the caller's device rows dst + k * stride, their
    /// lengths into the uint32 words at lens + 4 k (Program::frame, one item
    /// per packet).  Source and length come from the slot (buf + header,
    /// bytes - header); flow <= kFrameMaxFlow: a kFrameOriginal header
    /// (frame_write_header) goes before the payload, kFrameNone: none.  A packet
    /// outside the unacknowledged window (never added, or removed) is absent:
    /// its item writes only a zero length.  Never waits.  results[k]
    /// (optional) = Success / NeedMoreData, *queued = packets present.
    /// InvalidInput, with nothing queued, when header + payload of a present
    /// packet exceed the stride.
    static constexpr unsigned kFrameNone = 0xffffffffu;
    SiameseResult deliver_range(unsigned firstNum, unsigned count, unsigned flow, uint64_t dst, uint64_t stride,
                                uint64_t lens, SiameseResult* results, unsigned* queued);
    /// sgpu_encoder_pack_frames: queue the present originals firstNum, firstNum
    /// + 1, ... (originalCount of them, ascending) and then the recovery
    /// packets rec[0, recCount) as frames for `flow`, several to a row of
    /// `stride` bytes at dst + row * stride.  The layout rule: a cursor (row,
    /// off) from (0, 0); a frame of T = header + data bytes with off + T >
    /// stride moves to (row + 1, 0); it is placed at off, then off =
    /// align16(off + T).  One Program::frame item per frame covers its slot
    /// (to the next frame of the row, the row's last to the row's end: rows are
    /// written whole); the last item of a row also writes the row's length
    /// word lens + 4 row = its offset + T (FrameItem::lenBase), and rows
    /// [*rows, maxRows) get a length-only item (zero).  An absent original
    /// takes no space (results[k] = NeedMoreData).  Never waits.
    /// InvalidInput, with nothing queued: a frame with T > stride, a recovery
    /// packet that is not among this encoder's current output, or more rows
    /// than maxRows (*rows = the rows needed).
    struct PackRecovery
    {
        uint64_t data;
        uint32_t bytes;
    };
    SiameseResult pack_frames(unsigned flow, unsigned firstNum, unsigned originalCount, const PackRecovery* rec,
                              unsigned recCount, uint64_t dst, uint64_t stride, unsigned maxRows, uint64_t lens,
                              SiameseResult* results, unsigned* rows, unsigned* frames);
    /// sgpu_encoder_retransmit_frames: retransmit() until it answers
    /// NeedMoreData or maxPackets packets were returned, each queued as a
    /// kFrameOriginal frame for `flow` into rows of `stride` bytes at dst + row *
    /// stride, laid out by pack_frames' cursor rule (frames.h pack_plan makes the
    /// layout from the lengths, Program::frame places it: rows written whole,
    /// length words as pack_frames writes them, zero for rows [*rows, maxRows)).
    /// retransmit() stamps the packet it returns, so none is asked for that
    /// could not be placed: before each call a frame of the longest original of
    /// the unacknowledged window must fit the rows that are left, or the call
    /// ends with Success and what it has; when such a frame does not fit
    /// `stride` at all, InvalidInput with nothing consumed and nothing queued.
    /// packetNums[i] (optional) = frame i's PacketNum.  A result of retransmit()
    /// other than Success and NeedMoreData is returned, nothing being queued.
    SiameseResult retransmit_frames(unsigned flow, unsigned maxPackets, uint64_t dst, uint64_t stride,
                                    unsigned maxRows, uint64_t lens, unsigned* packetNums, unsigned* rows,
                                    unsigned* frames);
    /// Generate the next recovery packet (device ops queued, not flushed).
    SiameseResult encode(EncodeOut& out);
    /// `count` encode() calls in one (sgpu_encode_range): out[k] as the k-th
    /// call fills it, stopping at the first call that does not succeed (its
    /// result returned, Success otherwise); *produced = packets made.  Every
    /// packet's buffer stays valid until the next encode call.
    SiameseResult encode_range(EncodeOut* out, unsigned count, unsigned* produced);
    /// encode_range continued: the packets of the call before are kept too
    /// (one sgpu_encode_range made in several chunks).
    SiameseResult encode_range_more(EncodeOut* out, unsigned count, unsigned* produced);
    SiameseResult stats(uint64_t* out, unsigned count);
    /// ARQ: siamese_encoder_ack / siamese_encoder_retransmit (arq.cpp)
    SiameseResult acknowledge(const uint8_t* data, unsigned bytes, unsigned& nextExpectedOut);
    SiameseResult retransmit(SiameseOriginalPacket& out);

    /// Disabled: this instance failed (sticky), or the device did (Engine::failed).
    bool disabled() const { return dead(); }
    bool dead() const { return disabled_ || eng_->failed(); }
    uint64_t stat(unsigned i) const { return stats_[i]; }

private:
    // window (reference EncoderPacketWindow)
    /// Why a uniform subwindow's records were written out (slot counters).
    enum DemoteCause
    {
        kDemoteAdd,      // a single add, or a range add the fast path does not take
        kDemoteLength,   // a range add of another length or column sequence
        kDemoteStride,   // a symbol larger than the slab's slots
        kDemoteStamp,    // a range add of the same shape at another send time
        kDemoteArq,      // a retransmission stamps one element
        kDemoteOther,    // any other reader or writer of slot records
        kDemoteCauses
    };
    /// The element's slot record, for code that reads or writes records: a
    /// uniform subwindow is demoted first.
    EncSlot& slot(unsigned element, DemoteCause cause = kDemoteOther)
    {
        EncSubwindow* sw = subwindows_[element / kSubwindow].get();
        if (sw->uni.mask)
            demote(sw, cause);
        sw->clean = false;
        return sw->slot[element % kSubwindow];
    }
    /// What an element's record says, read from the descriptor where the
    /// subwindow is uniform (never demotes).
    struct SlotView
    {
        uint8_t* ptr = nullptr;
        unsigned bytes = 0, column = 0, header = 0;
        uint32_t lastSend = 0;
        uint64_t addr() const { return (uint64_t)(uintptr_t)ptr; }
    };
    SlotView peek(unsigned element) const
    {
        const EncSubwindow& sw = *subwindows_[element / kSubwindow];
        const unsigned bit = element % kSubwindow;
        SlotView v;
        if (sw.uni.mask >> bit & 1u) {
            v.ptr = sw.slab.buf.ptr + (size_t)bit * sw.slab.stride;
            v.bytes = sw.uni.bytes;
            v.column = column_add(sw.uni.first, bit);
            v.header = sw.uni.header;
            v.lastSend = sw.uni.stamp;
        } else {
            const EncSlot& s = sw.slot[bit];
            v.ptr = s.buf.ptr;
            v.bytes = s.bytes;
            v.column = s.column;
            v.header = s.header;
            v.lastSend = s.lastSend;
        }
        return v;
    }
    /// Write the records of a uniform subwindow's slots from its descriptor:
    /// afterwards it is what the per-element code would have built.
    void demote(EncSubwindow* sw, DemoteCause cause);
    /// Slots [bit, bit + m) of a subwindow as a mask.
    static uint64_t run_bits(unsigned bit, unsigned m) { return (m >= 64 ? ~0ull : (1ull << m) - 1) << bit; }
    /// add_range: may the m originals of `need` bytes from `element` on (one
    /// subwindow's, the first with `column`) be added through the descriptor?
    /// A uniform subwindow they do not continue is demoted here.
    bool uniform_takes(EncSubwindow* sw, unsigned element, unsigned m, unsigned need, unsigned h, unsigned column,
                       uint32_t stamp);
    /// ... then, the first's slab slot taken: the descriptor and, in bulk,
    /// what take_element and fill_slot do for each of them.
    void add_uniform(EncSubwindow* sw, unsigned element, unsigned m, unsigned need, unsigned h, unsigned bytes,
                     unsigned column, uint32_t stamp);
    /// The slab of a subwindow leaving the window goes back to the arena; the
    /// records of slab slots forget their buffers (none when it is uniform).
    void release_subwindow(EncSubwindow* sw);
#ifdef SGPU_SLOT_CHECK
    void slot_check(const EncSubwindow* sw, const char* where) const;
    /// What the per-element code makes of add_uniform's originals (their
    /// records go into the shadow), compared after it.
    struct AddExpect
    {
        unsigned nextColumn, longest, laneLongest[kLanes], count;
        uint32_t stale;
        uint64_t oc, ob;
        size_t subs;
    };
    AddExpect slot_check_add(EncSubwindow* sw, unsigned element, unsigned m, const unsigned* lens, unsigned fixedBytes,
                             uint32_t stamp);
    void slot_check_added(const AddExpect& x) const;
    [[noreturn]] static void slot_check_failed(const char* where, const char* what, unsigned bit);
#endif
    unsigned column_to_element(unsigned c) const { return column_sub(c, columnStart_); }
    unsigned element_to_column(unsigned e) const { return column_add(e, columnStart_); }
    unsigned next_lane_element(unsigned element, unsigned lane) const
    {
        unsigned e = element - (element % kLanes) + lane;
        return e < element ? e + kLanes : e;
    }
    unsigned unacked() const { return count_ - firstUnremoved_; }
    /// The window bookkeeping of one add (reference :85-161) up to its slot:
    /// the element the packet takes (its column is nextColumn_ before).
    unsigned take_element();
    /// Give element's slot a destination for `need` bytes: its slab slot, or
    /// a buffer of its own.  False on an arena failure (the encoder is then
    /// disabled).
    bool place(unsigned element, unsigned need);
    /// The slot's fields and the window's lengths after its symbol is queued.
    void fill_slot(EncSlot& s, unsigned column, unsigned header, unsigned dataBytes, uint32_t stamp);
    void release_slot(EncSlot& s)
    {
        if (!s.inSlab)
            eng_->release(s.buf);
        s.buf = DevBuf();
        s.inSlab = false;
    }
    void start_window(unsigned column);
    void reset_sums(unsigned elementStart);
    void remove_elements();
    /// Lazily accumulate lane sums up to elementEnd; returns the sum.
    DevSum& get_sum(unsigned lane, unsigned sumIndex, unsigned elementEnd);
    void cover(unsigned lo, unsigned hi);   // row batch window covers [lo, hi)
    bool grow_sum(DevSum& s, unsigned bytes);

    SiameseResult single_row(EncodeOut& out);
    SiameseResult cauchy_row(EncodeOut& out);
    SiameseResult siamese_row(EncodeOut& out, unsigned row);
    /// siamese_row without the buffer (recovery_ holds it) and the
    /// accounting (*opBytes: the row's reference source bytes)
    SiameseResult siamese_row_body(EncodeOut& out, unsigned row, uint64_t* opBytes);
    bool ensure_recovery(unsigned bytes);
    void finish_row(EncodeOut& out, const RowMeta& meta, unsigned payloadBytes,
                    bool footerWritten = false);
    void update_rto();
    SiameseResult retransmit_slot(EncSlot& s, SiameseOriginalPacket& out);
    AckState ack_;

    Engine* eng_;
    Program prog_;
    bool mirror_;
    bool disabled_ = false;

    std::vector<EncSubwindowPtr> subwindows_;
    struct SubwindowTable
    {
        std::vector<EncSubwindowPtr> v;
        std::vector<DevBuf> held;   // (recoveryHeld_'s capacity)
    };
    unsigned nextColumn_ = 0;
    unsigned count_ = 0;
    unsigned columnStart_ = 0;
    unsigned longest_ = 0;
    unsigned firstUnremoved_ = 0;
    unsigned sumStart_ = 0, sumEnd_ = 0, sumColumnStart_ = 0, sumErased_ = 0;

    struct Lane
    {
        unsigned next[kSums];
        DevSum sum[kSums];
        unsigned longest = 0;
    } lanes_[kLanes];

    // sums (bit lane*3 + s) that may lag the window: set when an original
    // lands in their lane or the sums restart, cleared once a row folds them
    static constexpr uint32_t kAllSums = (1u << kRowSums) - 1;
    uint32_t staleSums_ = kAllSums;
    // the sums as rows read them (WinEntry per bit), valid unless stale
    WinEntry sumTable_[kRowSums];
    uint32_t sumPresent_ = 0;   // sums holding bytes
    bool sumTableStale_ = true;
    uint64_t sumTableVersion_ = 0;   // Program::rows_row's tag of sumTable_ as last rebuilt
    uint32_t sumClip_[kRowSums] = {};   // min(sum bytes, sumClipBytes_): reference source bytes
    unsigned sumClipBytes_ = ~0u;       // the row length sumClip_ was made for
    bool lastRowSiamese_ = false;       // the last encode() made a Siamese row

    DevBuf recovery_;          // reused recovery packet buffer
    std::vector<DevBuf> recoveryHeld_;   // encode_range's earlier packets (released by the next encode)
    unsigned nextRow_ = 0;
    unsigned nextParityColumn_ = 0;
    unsigned nextCauchyRow_ = 0;

    uint64_t stats_[SiameseEncoderStats_Count] = {};

    // slot counters of this encoder (summed at teardown, printed at exit with
    // SIAMESE_AMD_SLOT_COUNTS)
    unsigned uniformEntered_ = 0, slotWrites_ = 0;
    unsigned demotions_[kDemoteCauses] = {};
};

} // namespace sgpu
