// encoder.cpp -- see encoder.h.  Line citations are to the reference
// SiameseEncoder.cpp unless stated otherwise.
#include "encoder.h"
#include "frames.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sgpu {

namespace {

// Slot bookkeeping of all encoders of the process, printed at exit when
// SIAMESE_AMD_SLOT_COUNTS is set (read once): subwindows that entered the
// uniform state, demotions by cause, slot records written (by the
// per-element code and by demotions).  Each encoder counts for itself and
// adds its counts here when it is freed.
constexpr unsigned kSlotCauses = 6;
const char* const kSlotCauseNames[kSlotCauses] = {"add", "length", "stride", "stamp", "arq", "other"};
struct SlotCounts
{
    const bool on = std::getenv("SIAMESE_AMD_SLOT_COUNTS") != nullptr;
    std::atomic<uint64_t> encoders{0}, uniform{0}, writes{0};
    std::atomic<uint64_t> demote[kSlotCauses] = {};
    ~SlotCounts()
    {
        if (!on)
            return;
        std::fprintf(stderr, "slot counts: encoders %llu enc_uniform %llu enc_slot_writes %llu",
                     (unsigned long long)encoders.load(), (unsigned long long)uniform.load(),
                     (unsigned long long)writes.load());
        for (unsigned c = 0; c < kSlotCauses; ++c)
            std::fprintf(stderr, " enc_demote_%s %llu", kSlotCauseNames[c], (unsigned long long)demote[c].load());
        std::fprintf(stderr, "\n");
    }
} g_slots;

} // namespace

EncoderCore::EncoderCore(Engine* eng, bool hostMirror) : eng_(eng), prog_(eng, 0), mirror_(hostMirror)
{
    // Window starts cleared (:63-82)
    for (unsigned l = 0; l < kLanes; ++l)
        for (unsigned s = 0; s < kSums; ++s)
            lanes_[l].next[s] = l;
    // the subwindow table's capacity comes from an encoder freed on this
    // thread (see DecoderCore::Spare)
    if (SubwindowTable* t = CapStash<SubwindowTable>::take()) {
        subwindows_.swap(t->v);
        recoveryHeld_.swap(t->held);
        CapStash<SubwindowTable>::put_shell(t);
    }
}

EncoderCore::~EncoderCore()
{
    // one pass per subwindow: release owned buffers and leave the slots
    // fresh for the pool (EncSubwindowRecycle skips a clean subwindow)
    // (a uniform subwindow, or one never written, has fresh slots already)
    for (auto& sw : subwindows_) {
        if (sw->uni.mask) {
#ifdef SGPU_SLOT_CHECK
            slot_check(sw.get(), "teardown");
            for (EncSlot& s : sw->shadow)
                s = EncSlot();
#endif
            sw->uni = EncUniform();
        }
        if (!sw->clean)
            for (EncSlot& s : sw->slot) {
                if (!s.inSlab)
                    eng_->release(s.buf);
                s.buf = DevBuf();
                s.inSlab = false;
                s.bytes = s.column = s.header = 0;
                s.lastSend = 0;
                if (s.hostp)
                    s.hostp->clear();
            }
        eng_->slab_release(sw->slab);
        sw->slab = Slab();
        sw->clean = true;
    }
    static_assert(kDemoteCauses == kSlotCauses, "a name for every cause");
    if (g_slots.on) {
        g_slots.encoders.fetch_add(1, std::memory_order_relaxed);
        g_slots.uniform.fetch_add(uniformEntered_, std::memory_order_relaxed);
        g_slots.writes.fetch_add(slotWrites_, std::memory_order_relaxed);
        for (unsigned c = 0; c < kSlotCauses; ++c)
            g_slots.demote[c].fetch_add(demotions_[c], std::memory_order_relaxed);
    }
    for (Lane& l : lanes_)
        for (DevSum& s : l.sum)
            eng_->release(s.buf);
    eng_->release(recovery_);
    for (DevBuf& b : recoveryHeld_)
        eng_->release(b);
    subwindows_.clear();   // (subwindows go back to their own pool)
    recoveryHeld_.clear();
    SubwindowTable* t = CapStash<SubwindowTable>::shell();
    subwindows_.swap(t->v);
    recoveryHeld_.swap(t->held);
    CapStash<SubwindowTable>::give(t);
}

// ---------------------------------------------------------------------------
// Window bookkeeping

unsigned EncoderCore::take_element()
{
    // :85-161
    const unsigned column = nextColumn_;
    unsigned element = count_;

    // Keep one lane-width of spare slots ahead of the last subwindow (:108-118)
    if (element + kLanes >= subwindows_.size() * kSubwindow) {
        subwindows_.emplace_back(ObjPool<EncSubwindow>::get());
        subwindows_.back()->clean = true;   // (the pool's objects are fresh)
    }

    if (count_ > 0)
        ++count_;
    else {
        element = column % kLanes;
        start_window(column);
    }
    return element;
}

void EncoderCore::demote(EncSubwindow* sw, DemoteCause cause)
{
#ifdef SGPU_SLOT_CHECK
    slot_check(sw, "demote");
    for (EncSlot& s : sw->shadow)
        s = EncSlot();
#endif
    const EncUniform u = sw->uni;
    for (uint64_t m = u.mask; m; m &= m - 1) {
        const unsigned bit = (unsigned)__builtin_ctzll(m);
        EncSlot& s = sw->slot[bit];
        s.buf.ptr = sw->slab.buf.ptr + (size_t)bit * sw->slab.stride;
        s.buf.cap = sw->slab.stride;
        s.inSlab = true;
        s.bytes = u.bytes;
        s.header = u.header;
        s.column = column_add(u.first, bit);
        s.lastSend = u.stamp;
    }
    sw->uni = EncUniform();
    sw->clean = false;
    slotWrites_ += (unsigned)__builtin_popcountll(u.mask);
    ++demotions_[cause];
}

void EncoderCore::release_subwindow(EncSubwindow* sw)
{
    if (sw->uni.mask) {
#ifdef SGPU_SLOT_CHECK
        slot_check(sw, "release");
        for (EncSlot& s : sw->shadow)
            s = EncSlot();
#endif
        sw->uni = EncUniform();
    } else if (!sw->clean) {
        // (its records keep their lengths and columns, as they always have,
        // and `clean` stays false: a subwindow that was demoted or filled
        // element by element is per-element until the encoder is freed.
        // Intended: making it fresh again would cost this walk 64 more
        // record writes for a case the headline never meets.)
        for (EncSlot& s : sw->slot)
            if (s.inSlab) {
                s.buf = DevBuf();
                s.inSlab = false;
            }
    }
    eng_->slab_release(sw->slab);
}

#ifdef SGPU_SLOT_CHECK
void EncoderCore::slot_check_failed(const char* where, const char* what, unsigned bit)
{
    std::fprintf(stderr, "SGPU_SLOT_CHECK: encoder %s: slot %u: %s differs from the per-element record\n", where, bit,
                 what);
    std::abort();
}

void EncoderCore::slot_check(const EncSubwindow* sw, const char* where) const
{
    const EncUniform& u = sw->uni;
    if (!sw->clean)
        slot_check_failed(where, "clean", 0);
    for (unsigned bit = 0; bit < kSubwindow; ++bit) {
        const EncSlot& sh = sw->shadow[bit];
        const EncSlot& real = sw->slot[bit];
        if (real.buf.ptr || real.buf.cap || real.inSlab || real.bytes || real.column || real.header ||
            real.lastSend)
            slot_check_failed(where, "fresh slot[]", bit);
        if (!(u.mask >> bit & 1u)) {
            if (sh.buf.ptr || sh.bytes || sh.inSlab)
                slot_check_failed(where, "mask", bit);
            continue;
        }
        if (sh.buf.ptr != sw->slab.buf.ptr + (size_t)bit * sw->slab.stride)
            slot_check_failed(where, "buf.ptr", bit);
        if (sh.buf.cap != sw->slab.stride)
            slot_check_failed(where, "buf.cap", bit);
        if (!sh.inSlab)
            slot_check_failed(where, "inSlab", bit);
        if (!(sw->slab.used >> bit & 1u))
            slot_check_failed(where, "slab.used", bit);
        if (sh.bytes != u.bytes)
            slot_check_failed(where, "bytes", bit);
        if (sh.header != u.header)
            slot_check_failed(where, "header", bit);
        if (sh.column != column_add(u.first, bit))
            slot_check_failed(where, "column", bit);
        if (sh.lastSend != u.stamp)
            slot_check_failed(where, "lastSend", bit);
    }
}
#endif

bool EncoderCore::place(unsigned element, unsigned need)
{
    EncSubwindow* sw = subwindows_[element / kSubwindow].get();
    if (sw->uni.mask)
        demote(sw, kDemoteAdd);
    sw->clean = false;
    ++slotWrites_;
    EncSlot& s = sw->slot[element % kSubwindow];
    release_slot(s);
    bool failed = false;
    s.buf = eng_->slab_slot(sw->slab, element % kSubwindow, need, &failed);
    s.inSlab = (bool)s.buf;
    if (!s.buf && !failed)
        s.buf = eng_->alloc(need);
    if (!s.buf) {
        disabled_ = true;
        return false;
    }
    return true;
}

void EncoderCore::fill_slot(EncSlot& s, unsigned column, unsigned header, unsigned dataBytes, uint32_t stamp)
{
    s.header = header;
    s.bytes = header + dataBytes;
    s.column = column;
    s.lastSend = stamp;

    nextColumn_ = column_add(nextColumn_, 1);

    staleSums_ |= 7u << (column % kLanes * kSums);
    Lane& lane = lanes_[column % kLanes];
    if (lane.longest < s.bytes)
        lane.longest = s.bytes;
    if (longest_ < s.bytes)
        longest_ = s.bytes;

    stats_[SiameseEncoderStats_OriginalCount]++;
    stats_[SiameseEncoderStats_OriginalBytes] += dataBytes;
}

SiameseResult EncoderCore::add(SiameseOriginalPacket& packet, uint64_t deviceSrc)
{
    // :85-161
    if (dead())
        return Siamese_Disabled;
    if (remaining_slots() == 0)
        return Siamese_MaxPacketsReached;

    const unsigned column = nextColumn_;
    packet.PacketNum = column;
    const unsigned element = take_element();

    uint8_t hdr[kMaxLengthPrefix];
    const unsigned h = write_length_prefix(packet.DataBytes, hdr);
    if (!place(element, h + packet.DataBytes))
        return Siamese_Disabled;
    EncSlot& s = slot(element);
    if (deviceSrc)
        prog_.ingest_device(s.buf, deviceSrc, packet.DataBytes, hdr, h);
    else
        prog_.ingest_host(s.buf, packet.Data, packet.DataBytes, hdr, h);
    if (mirror_) {
        s.host().resize(h + packet.DataBytes);
        std::memcpy(s.host().data(), hdr, h);
        std::memcpy(s.host().data() + h, packet.Data, packet.DataBytes);
    }
    fill_slot(s, column, h, packet.DataBytes, (uint32_t)now_msec());
    return Siamese_Success;
}

bool EncoderCore::uniform_takes(EncSubwindow* sw, unsigned element, unsigned m, unsigned need, unsigned h,
                                unsigned column, uint32_t stamp)
{
    if (mirror_ || !sw->clean)
        return false;
    const unsigned bit = element % kSubwindow;
    const EncUniform& u = sw->uni;
    if (!u.mask)   // fresh: no slab yet, and one that slab_slot will grant
        return !sw->slab.buf && slab_stride(need) != 0;
    // (one cause per demotion, the first that applies)
    if (need > sw->slab.stride)
        demote(sw, kDemoteStride);
    else if (u.bytes != need || u.header != h || column_add(u.first, bit) != column)
        demote(sw, kDemoteLength);
    else if (u.stamp != stamp)
        demote(sw, kDemoteStamp);
    else if (sw->slab.used & run_bits(bit, m))
        demote(sw, kDemoteAdd);
    else
        return true;
    return false;
}

void EncoderCore::add_uniform(EncSubwindow* sw, unsigned element, unsigned m, unsigned need, unsigned h,
                              unsigned bytes, unsigned column, uint32_t stamp)
{
    const unsigned bit = element % kSubwindow;
    const uint64_t bits = run_bits(bit, m);
    sw->slab.used |= bits;
    if (!sw->uni.mask) {
        sw->uni.bytes = need;
        sw->uni.header = h;
        sw->uni.first = column_sub(column, bit);
        sw->uni.stamp = stamp;
        ++uniformEntered_;
    }
    sw->uni.mask |= bits;
    // what fill_slot and take_element do for each of the m
    nextColumn_ = column_add(nextColumn_, m);
    for (unsigned j = 0; j < std::min(m, kLanes); ++j) {
        const unsigned l = (column + j) % kLanes;
        staleSums_ |= 7u << (l * kSums);
        if (lanes_[l].longest < need)
            lanes_[l].longest = need;
    }
    if (longest_ < need)
        longest_ = need;
    stats_[SiameseEncoderStats_OriginalCount] += m;
    stats_[SiameseEncoderStats_OriginalBytes] += (uint64_t)m * bytes;
    count_ += m - 1;
    // (take_element's growth rule: of the elements behind the first, only
    // the subwindow's last ones can ask for another, and for one only)
    if (m > 1 && element + m - 1 + kLanes >= subwindows_.size() * kSubwindow) {
        subwindows_.emplace_back(ObjPool<EncSubwindow>::get());
        subwindows_.back()->clean = true;
    }
}

#ifdef SGPU_SLOT_CHECK
EncoderCore::AddExpect EncoderCore::slot_check_add(EncSubwindow* sw, unsigned element, unsigned m, const unsigned* lens,
                                                   unsigned fixedBytes, uint32_t stamp)
{
    // the per-element code on a copy of the window's lengths and counters
    // (the first element's take_element has run), its records into the shadow
    AddExpect x;
    x.nextColumn = nextColumn_;
    x.stale = staleSums_;
    x.longest = longest_;
    for (unsigned l = 0; l < kLanes; ++l)
        x.laneLongest[l] = lanes_[l].longest;
    x.oc = stats_[SiameseEncoderStats_OriginalCount];
    x.ob = stats_[SiameseEncoderStats_OriginalBytes];
    x.count = count_;
    x.subs = subwindows_.size();
    const unsigned bit = element % kSubwindow;
    for (unsigned j = 0; j < m; ++j) {
        const unsigned len = lens ? lens[j] : fixedBytes;
        uint8_t hd[kMaxLengthPrefix];
        const unsigned hj = write_length_prefix(len, hd);
        const unsigned cj = x.nextColumn;
        if (j > 0) {
            if (x.count + kLanes >= x.subs * kSubwindow)
                ++x.subs;
            ++x.count;
        }
        EncSlot& sh = sw->shadow[bit + j];
        if (sh.buf.ptr || sh.bytes)
            slot_check_failed("add_range", "slot written before", bit + j);
        sh.buf.ptr = sw->slab.buf.ptr + (size_t)(bit + j) * sw->slab.stride;
        sh.buf.cap = sw->slab.stride;
        sh.inSlab = true;
        sh.header = hj;
        sh.bytes = hj + len;
        sh.column = cj;
        sh.lastSend = stamp;
        x.nextColumn = column_add(x.nextColumn, 1);
        x.stale |= 7u << (cj % kLanes * kSums);
        x.laneLongest[cj % kLanes] = std::max(x.laneLongest[cj % kLanes], sh.bytes);
        x.longest = std::max(x.longest, sh.bytes);
        ++x.oc;
        x.ob += len;
        if ((element + j) % kLanes != cj % kLanes)
            slot_check_failed("add_range", "element % 8 == column % 8", bit + j);
    }
    return x;
}

void EncoderCore::slot_check_added(const AddExpect& x) const
{
    if (x.nextColumn != nextColumn_ || x.stale != staleSums_ || x.longest != longest_ ||
        x.oc != stats_[SiameseEncoderStats_OriginalCount] || x.ob != stats_[SiameseEncoderStats_OriginalBytes] ||
        x.count != count_ || x.subs != subwindows_.size())
        slot_check_failed("add_range", "window bookkeeping", 0);
    for (unsigned l = 0; l < kLanes; ++l)
        if (x.laneLongest[l] != lanes_[l].longest)
            slot_check_failed("add_range", "lane longest", l);
}
#endif

SiameseResult EncoderCore::add_range(uint64_t src, uint32_t srcStride, const unsigned* lens, unsigned fixedBytes,
                                     unsigned count, unsigned* firstNum, unsigned* added)
{
    *added = 0;
    *firstNum = nextColumn_;
    if (dead())
        return Siamese_Disabled;
    // one timestamp for the call (ARQ's RTO is milliseconds)
    const uint32_t stamp = count ? (uint32_t)now_msec() : 0;
    // the open ingest run: symbols of one length into consecutive slots
    struct
    {
        uint64_t dst = 0, src = 0;
        uint32_t stride = 0, n = 0, bytes = 0, h = 0;
        uint8_t hdr[kMaxLengthPrefix] = {};
    } run;
    auto close_run = [&] {
        if (run.n)
            prog_.ingest_run(run.dst, run.stride, run.src, srcStride, run.n, run.bytes, run.hdr, run.h);
        run.n = 0;
    };
    // `n` symbols of one length into consecutive slots of `cap` bytes from
    // dst: the runs the per-element code makes of them (<= kIngestRunMax each)
    auto append = [&](uint64_t dst, uint32_t cap, uint64_t from, unsigned bytes, unsigned h, const uint8_t* hdr,
                      unsigned n) {
        while (n) {
            if (!(run.n && run.bytes == bytes && run.n < kIngestRunMax && cap == run.stride &&
                  dst == run.dst + (uint64_t)run.n * run.stride && from == run.src + (uint64_t)run.n * srcStride)) {
                close_run();
                run.dst = dst;
                run.src = from;
                run.stride = cap;
                run.bytes = bytes;
                run.h = h;
                std::memcpy(run.hdr, hdr, kMaxLengthPrefix);
            }
            const unsigned t = std::min<unsigned>(n, kIngestRunMax - run.n);
            run.n += t;
            dst += (uint64_t)t * cap;
            from += (uint64_t)t * srcStride;
            n -= t;
        }
    };
    SiameseResult res = Siamese_Success;
    for (unsigned k = 0; k < count;) {
        const unsigned bytes = lens ? lens[k] : fixedBytes;
        if (bytes == 0 || bytes > SIAMESE_MAX_PACKET_BYTES) {
            res = Siamese_InvalidInput;
            break;
        }
        if (remaining_slots() == 0) {
            res = Siamese_MaxPacketsReached;
            break;
        }
        const unsigned column = nextColumn_;
        const unsigned element = take_element();
        uint8_t hdr[kMaxLengthPrefix] = {};
        const unsigned h = write_length_prefix(bytes, hdr);
        const unsigned need = h + bytes;
        const uint64_t from = src + (uint64_t)k * srcStride;

        // The uniform path: this original and those behind it of the same
        // length, as far as the subwindow, the window's limit and the call go
        EncSubwindow* sw = subwindows_[element / kSubwindow].get();
        unsigned m = std::min(std::min(count - k, kSubwindow - element % kSubwindow), 1 + remaining_slots());
        if (lens)
            for (unsigned j = 1; j < m; ++j)
                if (lens[k + j] != bytes) {
                    m = j;
                    break;
                }
        if (uniform_takes(sw, element, m, need, h, column, stamp)) {
            bool failed = false;
            const DevBuf b = eng_->slab_slot(sw->slab, element % kSubwindow, need, &failed);
            if (failed) {
                disabled_ = true;
                res = Siamese_Disabled;
                break;
            }
            if (b) {
#ifdef SGPU_SLOT_CHECK
                const AddExpect expect = slot_check_add(sw, element, m, lens ? lens + k : nullptr, fixedBytes, stamp);
#endif
                add_uniform(sw, element, m, need, h, bytes, column, stamp);
#ifdef SGPU_SLOT_CHECK
                slot_check_added(expect);
#endif
                append(b.addr(), b.cap, from, bytes, h, hdr, m);
                k += m;
                *added += m;
                continue;
            }
        }

        // one element as add() places it
        if (!place(element, need)) {
            res = Siamese_Disabled;
            break;
        }
        EncSlot& s = slot(element);
        append(s.buf.addr(), s.buf.cap, from, bytes, h, hdr, 1);
        fill_slot(s, column, h, bytes, stamp);
        ++*added;
        ++k;
    }
    close_run();
    return res;
}

void EncoderCore::start_window(unsigned column)
{
    // :163-181 -- element % 8 == column % 8 is an invariant of the window
    const unsigned element = column % kLanes;
    // window indices start over below: close the open row batch first, or a
    // row of the new window made in the same submission as one of the old
    // would find its elements in the old window's snapshot (remove_elements)
    prog_.rows_seal();
    // every element of the old window was acknowledged: slabs start afresh
    for (auto& sw : subwindows_)
        release_subwindow(sw.get());
    columnStart_ = column - element;
    sumStart_ = element;
    sumEnd_ = element;
    firstUnremoved_ = element;
    count_ = element + 1;
    longest_ = 0;
    for (Lane& l : lanes_)
        l.longest = 0;
    staleSums_ = kAllSums;
    sumTableStale_ = true;
}

void EncoderCore::remove_before(unsigned firstKeptColumn)
{
    // :183-216
    if (dead())
        return;
    const unsigned element = column_to_element(firstKeptColumn);
    if (element >= count_) {
        if (!column_delta_negative(element))
            count_ = 0; // everything acknowledged
        return;
    }
    if (firstUnremoved_ < element)
        firstUnremoved_ = element;
}

void EncoderCore::reset_sums(unsigned elementStart)
{
    // :218-237
    for (unsigned l = 0; l < kLanes; ++l) {
        const unsigned first = next_lane_element(elementStart, l);
        for (unsigned s = 0; s < kSums; ++s) {
            lanes_[l].next[s] = first;
            lanes_[l].sum[s].bytes = 0;
            lanes_[l].sum[s].devValid = 0;
        }
    }
    sumStart_ = elementStart;
    sumEnd_ = elementStart;
    sumColumnStart_ = element_to_column(elementStart);
    sumErased_ = 0;
    staleSums_ = kAllSums;
    sumTableStale_ = true;
}

void EncoderCore::remove_elements()
{
    // :239-357 -- drop whole subwindows before FirstUnremovedElement
    const unsigned keptSub = firstUnremoved_ / kSubwindow;
    const unsigned removed = keptSub * kSubwindow;

    if (sumEnd_ > sumStart_) {
        // Roll the running sums past the removal point before the data goes
        for (unsigned l = 0; l < kLanes; ++l) {
            for (unsigned s = 0; s < kSums; ++s) {
                get_sum(l, s, removed);
                lanes_[l].next[s] -= removed;
            }
        }
        if (removed > sumStart_)
            sumErased_ += removed - sumStart_;
        sumEnd_ = sumEnd_ > removed ? sumEnd_ - removed : 0;
        sumStart_ = sumStart_ > removed ? sumStart_ - removed : 0;
    }

    // window indices shift below: close the open row batch first
    prog_.rows_seal();
    // Removed subwindows rotate to the back for reuse; their slabs go back
    // to the arena (after the flushes that read them)
    for (unsigned i = 0; i < keptSub; ++i)
        release_subwindow(subwindows_[i].get());
    std::rotate(subwindows_.begin(), subwindows_.begin() + keptSub, subwindows_.end());

    count_ -= removed;
    columnStart_ = element_to_column(removed);
    firstUnremoved_ -= removed;
    staleSums_ = kAllSums;
    sumTableStale_ = true;

    unsigned longest = 0;
    unsigned laneLongest[kLanes] = {0};
    for (unsigned e = firstUnremoved_; e < count_; ++e) {
        const unsigned b = peek(e).bytes;
        longest = std::max(longest, b);
        laneLongest[e % kLanes] = std::max(laneLongest[e % kLanes], b);
    }
    longest_ = longest;
    for (unsigned l = 0; l < kLanes; ++l)
        lanes_[l].longest = laneLongest[l];

    if (sumEnd_ <= sumStart_)
        reset_sums(firstUnremoved_);
}

bool EncoderCore::grow_sum(DevSum& s, unsigned bytes)
{
    if (bytes <= s.bytes)
        return true;
    if (bytes > s.buf.cap) {
        DevBuf nb = eng_->alloc(bytes);
        if (!nb) {
            disabled_ = true;
            return false;
        }
        if (s.devValid) {
            prog_.lc_begin(nb.addr(), s.devValid, 0);
            prog_.lc_term(s.buf.addr(), s.devValid, 1);
            prog_.lc_end();
        }
        eng_->release(s.buf);
        s.buf = nb;
    }
    s.bytes = bytes;
    return true;
}

void EncoderCore::cover(unsigned lo, unsigned hi)
{
    uint32_t from = hi;
    WinEntry* w = prog_.rows_window(lo, hi, &from);
    for (unsigned e = from; e < hi;) {
        // one subwindow's part of the snapshot: from its descriptor when
        // that describes all of it, else element by element
        const EncSubwindow* sw = subwindows_[e / kSubwindow].get();
        const unsigned bit = e % kSubwindow;
        const unsigned n = std::min(hi - e, kSubwindow - bit);
        const uint64_t bits = (n == kSubwindow ? ~0ull : (1ull << n) - 1) << bit;
#ifdef SGPU_SLOT_CHECK
        if (sw->uni.mask)
            slot_check(sw, "cover");
#endif
        if ((sw->uni.mask & bits) == bits) {
            uint64_t at = (uint64_t)(uintptr_t)sw->slab.buf.ptr + (uint64_t)bit * sw->slab.stride;
            for (unsigned j = 0; j < n; ++j, ++w, at += sw->slab.stride) {
                w->src = at;
                w->len = sw->uni.bytes;
                w->column = column_add(sw->uni.first, bit + j);
            }
        } else {
            for (unsigned j = 0; j < n; ++j, ++w) {
                const SlotView o = peek(e + j);
                w->src = o.addr();
                w->len = o.bytes;
                w->column = o.column;
            }
        }
        e += n;
    }
}

DevSum& EncoderCore::get_sum(unsigned lane, unsigned sumIndex, unsigned elementEnd)
{
    // :359-418 -- lazily fold this lane's new originals into the running sum.
    // Sum0 += X, Sum1 += CX*X, Sum2 += CX^2*X.  The terms and coefficients
    // are generated on the device from the row batch's window snapshot.
    Lane& L = lanes_[lane];
    DevSum& sum = L.sum[sumIndex];
    unsigned element = L.next[sumIndex];
    if (element >= elementEnd)
        return sum;

    // The sum grows to the longest original it covers.  L.longest bounds
    // every element of the lane from FirstUnremoved on; older (acknowledged)
    // elements are checked one by one.
    unsigned newBytes = std::max(sum.bytes, L.longest);
    const unsigned end = element + ((elementEnd - element + kLanes - 1) / kLanes) * kLanes;
    for (unsigned e = element; e < end && e < firstUnremoved_; e += kLanes)
        newBytes = std::max(newBytes, peek(e).bytes);
    if (!grow_sum(sum, newBytes))
        return sum;
    // reference source bytes (one add/muladd per original) are counted by
    // the device as it expands the update
    cover(std::min(element, std::min(sumStart_, firstUnremoved_)), end - kLanes + 1);
    prog_.rows_update(lane * kSums + sumIndex, sum.buf.addr(), sum.bytes, sum.devValid, sumIndex,
                      element, end);
    sum.devValid = sum.bytes;
    L.next[sumIndex] = end;
    return sum;
}

SiameseResult EncoderCore::get(SiameseOriginalPacket& packet)
{
    if (dead())
        return Siamese_Disabled;
    const unsigned element = column_to_element(packet.PacketNum);
    if (element >= count_ || peek(element).bytes == 0) {
        packet.Data = nullptr;
        packet.DataBytes = 0;
        return Siamese_NeedMoreData;
    }
    EncSlot& s = slot(element);
    packet.PacketNum = s.column;
    packet.Data = mirror_ ? s.host().data() + s.header : s.buf.ptr + s.header;
    packet.DataBytes = s.bytes - s.header;
    return Siamese_Success;
}

SiameseResult EncoderCore::deliver_range(unsigned firstNum, unsigned count, unsigned flow, uint64_t dst,
                                         uint64_t stride, uint64_t lens, SiameseResult* results, unsigned* queued)
{
    *queued = 0;
    if (dead())
        return Siamese_Disabled;
    const bool framed = flow != kFrameNone;
    // the unacknowledged window, as get() and remove_before() see it
    auto held = [&](unsigned column) -> const EncSlot* {
        const unsigned e = column_to_element(column);
        if (e >= count_ || e < firstUnremoved_)
            return nullptr;
        const EncSlot& s = slot(e);   // (demotes: delivery reads records)
        return s.bytes != 0 && s.column == column ? &s : nullptr;
    };
    // every length is known here: nothing is queued when a packet cannot fit
    for (unsigned k = 0; k < count; ++k)
        if (const EncSlot* s = held(column_add(firstNum, k))) {
            const unsigned n = s->bytes - s->header;
            if ((uint64_t)(framed ? frame_header_bytes(kFrameOriginal, n) : 0) + n > stride)
                return Siamese_InvalidInput;
        }
    for (unsigned k = 0; k < count; ++k) {
        const unsigned column = column_add(firstNum, k);
        const EncSlot* s = held(column);
        uint8_t hdr[kFrameMaxHeader] = {};
        unsigned h = 0, n = 0;
        if (s) {
            n = s->bytes - s->header;
            if (framed)
                h = frame_write_header(kFrameOriginal, flow, column, n, hdr);
        }
        prog_.frame(s ? s->buf.addr() + s->header : 0, n, hdr, h, dst + (uint64_t)k * stride,
                    lens + (uint64_t)k * 4, stride);
        if (results)
            results[k] = s ? Siamese_Success : Siamese_NeedMoreData;
        if (s)
            ++*queued;
    }
    return Siamese_Success;
}

SiameseResult EncoderCore::pack_frames(unsigned flow, unsigned firstNum, unsigned originalCount,
                                       const PackRecovery* rec, unsigned recCount, uint64_t dst, uint64_t stride,
                                       unsigned maxRows, uint64_t lens, SiameseResult* results, unsigned* rows,
                                       unsigned* frames)
{
    *rows = *frames = 0;
    if (dead())
        return Siamese_Disabled;
    struct Placed
    {
        uint64_t src;
        uint32_t bytes, hdrLen, column;
        uint64_t row, off;
        uint8_t hdr[kFrameMaxHeader];
    };
    std::vector<Placed> placed;
    placed.reserve((size_t)originalCount + recCount);
    uint64_t row = 0, off = 0;
    // the layout rule (encoder.h); false: the frame is longer than a row
    auto place = [&](unsigned type, unsigned column, uint64_t src, uint32_t n) {
        Placed p;
        std::memset(p.hdr, 0, sizeof(p.hdr));
        p.src = src;
        p.bytes = n;
        p.column = column;
        p.hdrLen = frame_write_header(type, flow, column, n, p.hdr);
        const uint64_t T = (uint64_t)p.hdrLen + n;
        if (T > stride)
            return false;
        if (off + T > stride) {
            ++row;
            off = 0;
        }
        p.row = row;
        p.off = off;
        off = (off + T + 15) & ~(uint64_t)15;
        placed.push_back(p);
        return true;
    };
    for (unsigned k = 0; k < originalCount; ++k) {
        // the unacknowledged window, as deliver_range() sees it
        const unsigned column = column_add(firstNum, k);
        const unsigned e = column_to_element(column);
        if (e >= count_ || e < firstUnremoved_)
            continue;
        const EncSlot& s = slot(e);
        if (s.bytes == 0 || s.column != column)
            continue;
        if (!place(kFrameOriginal, column, s.buf.addr() + s.header, s.bytes - s.header))
            return Siamese_InvalidInput;
    }
    const size_t originals = placed.size();
    for (unsigned k = 0; k < recCount; ++k) {
        bool mine = rec[k].data != 0 && recovery_ && rec[k].data == recovery_.addr();
        for (const DevBuf& b : recoveryHeld_)
            mine = mine || (rec[k].data != 0 && b && rec[k].data == b.addr());
        if (!mine || rec[k].bytes == 0 || rec[k].bytes > SIAMESE_MAX_PACKET_BYTES ||
            !place(kFrameRecovery, 0, rec[k].data, rec[k].bytes))
            return Siamese_InvalidInput;
    }
    const uint64_t need = placed.empty() ? 0 : row + 1;
    if (need > maxRows) {
        *rows = (unsigned)std::min<uint64_t>(need, 0xffffffffu);
        return Siamese_InvalidInput;
    }
    if (results) {
        size_t i = 0;
        for (unsigned k = 0; k < originalCount; ++k) {
            const bool present = i < originals && placed[i].column == column_add(firstNum, k);
            results[k] = present ? Siamese_Success : Siamese_NeedMoreData;
            i += present;
        }
    }
    for (size_t i = 0; i < placed.size(); ++i) {
        const Placed& p = placed[i];
        const bool last = i + 1 == placed.size() || placed[i + 1].row != p.row;
        const uint64_t span = (last ? stride : placed[i + 1].off) - p.off;
        prog_.frame(p.src, p.bytes, p.hdr, p.hdrLen, dst + p.row * stride + p.off, last ? lens + p.row * 4 : 0, span,
                    last ? (uint32_t)p.off : 0);
    }
    const uint8_t none[kFrameMaxHeader] = {};
    for (uint64_t r = need; r < maxRows; ++r)   // rows not used: only a zero length
        prog_.frame(0, 0, none, 0, dst + r * stride, lens + r * 4, stride);
    *rows = (unsigned)need;
    *frames = (unsigned)placed.size();
    return Siamese_Success;
}

SiameseResult EncoderCore::retransmit_frames(unsigned flow, unsigned maxPackets, uint64_t dst, uint64_t stride,
                                             unsigned maxRows, uint64_t lens, unsigned* packetNums, unsigned* rows,
                                             unsigned* frames)
{
    *rows = *frames = 0;
    if (dead())
        return Siamese_Disabled;
    // the longest frame a retransmission of the current window can need
    uint64_t worst = 0;
    for (unsigned e = firstUnremoved_; e < count_; ++e) {
        const SlotView s = peek(e);
        if (s.bytes > s.header) {
            const unsigned n = s.bytes - s.header;
            worst = std::max<uint64_t>(worst, (uint64_t)frame_header_bytes(kFrameOriginal, n) + n);
        }
    }
    if (worst > stride)
        return Siamese_InvalidInput;
    struct Sent
    {
        uint64_t src;
        uint32_t bytes, column;
        uint8_t prefix[kMaxLengthPrefix];   // the symbol prefix pack_plan reads the length from
        uint32_t cap;
    };
    std::vector<Sent> sent;
    uint64_t row = 0, off = 0;   // pack_frames' cursor
    while (sent.size() < maxPackets) {
        if ((off + worst > stride ? row + 1 : row) >= maxRows)
            break;   // the next packet might not fit: it is not asked for
        SiameseOriginalPacket p;
        const SiameseResult r = retransmit(p);
        if (r == Siamese_NeedMoreData)
            break;
        if (r != Siamese_Success)
            return r;
        Sent s;
        s.src = (uint64_t)(uintptr_t)p.Data;
        s.bytes = p.DataBytes;
        s.column = p.PacketNum;
        std::memset(s.prefix, 0, sizeof(s.prefix));
        s.cap = write_length_prefix(p.DataBytes, s.prefix) + p.DataBytes;
        sent.push_back(s);
        const uint64_t T = (uint64_t)frame_header_bytes(kFrameOriginal, p.DataBytes) + p.DataBytes;
        if (off + T > stride) {
            ++row;
            off = 0;
        }
        off = (off + T + 15) & ~(uint64_t)15;
    }
    const uint32_t count = (uint32_t)sent.size();
    std::vector<const uint8_t*> syms(count);
    std::vector<uint32_t> caps(count), rowLens(maxRows);
    std::vector<PlanRec> recs(count);
    for (uint32_t k = 0; k < count; ++k) {
        syms[k] = sent[k].prefix;
        caps[k] = sent[k].cap;
    }
    uint32_t info[4];
    pack_plan(syms.data(), caps.data(), count, stride, maxRows, recs.data(), rowLens.data(), info);
    for (uint32_t k = 0; k < count; ++k) {   // (every packet is a frame of a row below maxRows: checked before it was taken)
        const Sent& s = sent[k];
        uint8_t hdr[kFrameMaxHeader] = {};
        const unsigned h = frame_write_header(kFrameOriginal, flow, s.column, s.bytes, hdr);
        const bool last = k + 1 == count || recs[k + 1].row != recs[k].row;
        const uint64_t at = (uint64_t)recs[k].off16 << 4;
        prog_.frame(s.src, s.bytes, hdr, h, dst + recs[k].row * stride + at, last ? lens + (uint64_t)recs[k].row * 4 : 0,
                    (uint64_t)recs[k].span16 << 4, last ? (uint32_t)at : 0);
        if (packetNums)
            packetNums[k] = s.column;
    }
    const uint8_t none[kFrameMaxHeader] = {};
    for (uint64_t r = info[0]; r < maxRows; ++r)   // rows not used: only a zero length
        prog_.frame(0, 0, none, 0, dst + r * stride, lens + r * 4, stride);
    *rows = info[0];
    *frames = count;
    return Siamese_Success;
}

// ---------------------------------------------------------------------------
// Encode

bool EncoderCore::ensure_recovery(unsigned bytes)
{
    for (DevBuf& b : recoveryHeld_)
        eng_->release(b);
    recoveryHeld_.clear();
    // Every recovery packet gets a fresh buffer.  The previous one is
    // recycled only after the flush that produced it completes, so a decoder
    // that copies the packet later in the same flush (its own program, group
    // 1) still reads it intact, and consecutive rows carry no write-after-
    // read dependency through a shared buffer.
    eng_->release(recovery_);
    recovery_ = eng_->alloc(bytes);
    if (!recovery_) {
        disabled_ = true;
        return false;
    }
    return true;
}

void EncoderCore::finish_row(EncodeOut& out, const RowMeta& meta, unsigned payloadBytes,
                             bool footerWritten)
{
    out.meta = meta;
    out.footerBytes = write_footer(meta, out.footer);
    if (!footerWritten)
        prog_.literal(recovery_.addr(), payloadBytes, out.footer, out.footerBytes);
    out.buf = recovery_;
    out.bytes = payloadBytes + out.footerBytes;
    eng_->account(0, out.bytes);
    stats_[SiameseEncoderStats_RecoveryCount]++;
    stats_[SiameseEncoderStats_RecoveryBytes] += out.bytes;
}

SiameseResult EncoderCore::encode(EncodeOut& out)
{
    // :1146-1254
    lastRowSiamese_ = false;
    if (dead())
        return Siamese_Disabled;
    if (count_ == 0) {
        out.bytes = 0;
        return Siamese_NeedMoreData;
    }
    if (firstUnremoved_ >= kRemoveThreshold)
        remove_elements();

    const unsigned inFlight = unacked();
    if (inFlight == 1)
        return single_row(out);

    const unsigned sumWidthBound = count_ - sumStart_ + sumErased_;
    if (sumEnd_ <= sumStart_ || sumWidthBound >= kMaxPacketsInFlight) {
        if (inFlight <= kCauchyThreshold)
            return cauchy_row(out);
        reset_sums(firstUnremoved_);
    } else if (inFlight <= kSumResetThreshold || sumWidthBound <= kCauchyThreshold) {
        sumEnd_ = sumStart_; // stop the running sums
        return cauchy_row(out);
    }

    const unsigned row = nextRow_;
    if (++nextRow_ >= kRowValuePeriod)
        nextRow_ = 0;
    return siamese_row(out, row);
}

SiameseResult EncoderCore::encode_range(EncodeOut* out, unsigned count, unsigned* produced)
{
    for (DevBuf& b : recoveryHeld_)   // (the previous call's packets)
        eng_->release(b);
    recoveryHeld_.clear();
    return encode_range_more(out, count, produced);
}

SiameseResult EncoderCore::encode_range_more(EncodeOut* out, unsigned count, unsigned* produced)
{
    *produced = 0;
    std::vector<DevBuf> held;   // this call's packets before the last (and the chunks' before it)
    held.swap(recoveryHeld_);   // (capacity reused; ensure_recovery below finds none to release)
    SiameseResult r = Siamese_Success;
    // After a Siamese row, encode() would choose a Siamese row again: its
    // path depends on the window only, which no call of a range changes.
    // Those rows skip the per-call dispatch and share one accounting.
    bool siamese = false;
    uint64_t opAcc = 0, outAcc = 0;
    for (unsigned k = 0; k < count; ++k) {
        if (k > 0 || !held.empty() || *produced) {
            // keep the previous packet: ensure_recovery would release it
            held.push_back(recovery_);
            recovery_ = DevBuf();
        }
        if (siamese) {
            if (dead()) {
                r = Siamese_Disabled;
                break;
            }
            const unsigned row = nextRow_;
            if (++nextRow_ >= kRowValuePeriod)
                nextRow_ = 0;
            recovery_ = eng_->alloc(longest_ + kMaxFooterBytes);
            if (!recovery_) {
                disabled_ = true;
                r = Siamese_Disabled;
                break;
            }
            uint64_t ob = 0;
            r = siamese_row_body(out[k], row, &ob);
            if (r != Siamese_Success)
                break;
            opAcc += ob;
            outAcc += out[k].bytes;
        } else {
            r = encode(out[k]);
            if (r != Siamese_Success)
                break;
            siamese = lastRowSiamese_;
        }
        ++*produced;
    }
    eng_->account(opAcc, outAcc);
    recoveryHeld_.swap(held);
    return r;
}

SiameseResult EncoderCore::single_row(EncodeOut& out)
{
    // :1296-1329 -- the lone original itself, with a SumCount=1 footer
    const SlotView o = peek(firstUnremoved_);
    if (!ensure_recovery(o.bytes + kMaxFooterBytes))
        return Siamese_Disabled;
    prog_.lc_begin(recovery_.addr(), o.bytes, 0);
    prog_.lc_term(o.addr(), o.bytes, 1);
    prog_.lc_end();
    write_length_prefix(o.bytes - o.header, out.head);
    RowMeta m;
    m.sumCount = 1;
    m.ldpcCount = 1;
    m.columnStart = o.column;
    m.row = 0;
    finish_row(out, m, o.bytes);
    return Siamese_Success;
}

SiameseResult EncoderCore::cauchy_row(EncodeOut& out)
{
    // :1334-1441 -- parity row (Row 0) or Cauchy row over the unacked window
    const unsigned first = firstUnremoved_;
    if (!ensure_recovery(longest_ + kMaxFooterBytes))
        return Siamese_Disabled;
    const unsigned inFlight = unacked();
    RowMeta m;
    m.sumCount = inFlight;
    m.ldpcCount = inFlight;
    m.columnStart = element_to_column(first);

    unsigned used = 0;
    for (unsigned e = first; e < count_; ++e)
        used = std::max(used, peek(e).bytes);
    prog_.lc_begin(recovery_.addr(), used, 0);
    uint64_t opBytes = 0;

    const unsigned parityElement = column_to_element(nextParityColumn_);
    if (parityElement <= first || column_delta_negative(parityElement)) {
        nextParityColumn_ = column_add(m.columnStart, inFlight);
        m.row = 0;
        for (unsigned e = first; e < count_; ++e) {
            const SlotView o = peek(e);
            prog_.lc_term(o.addr(), o.bytes, 1);
            // the reference memcpy's the first parity column (no GF op)
            if (e > first)
                opBytes += o.bytes;
        }
    } else {
        const unsigned crow = nextCauchyRow_;
        m.row = crow + 1;
        if (++nextCauchyRow_ >= kCauchyMaxRows)
            nextCauchyRow_ = 0;
        unsigned ccol = m.columnStart % kCauchyMaxColumns;
        for (unsigned e = first; e < count_; ++e) {
            const SlotView o = peek(e);
            prog_.lc_term(o.addr(), o.bytes, cauchy_element(crow, ccol));
            opBytes += o.bytes;
            ccol = (ccol + 1) % kCauchyMaxColumns;
        }
    }
    prog_.lc_end();
    eng_->account(opBytes);
    finish_row(out, m, used);
    return Siamese_Success;
}

SiameseResult EncoderCore::siamese_row(EncodeOut& out, unsigned row)
{
    if (!ensure_recovery(longest_ + kMaxFooterBytes))
        return Siamese_Disabled;
    uint64_t opBytes = 0;
    const SiameseResult r = siamese_row_body(out, row, &opBytes);
    if (r == Siamese_Success)
        eng_->account(opBytes, out.bytes);
    return r;
}

SiameseResult EncoderCore::siamese_row_body(EncodeOut& out, unsigned row, uint64_t* opBytesOut)
{
    const unsigned recoveryBytes = longest_;

    // Dense part (:1046-1098): opcode bits 0-2 feed the row, 3-5 the product.
    // The lane sums are brought up to date first (their own ops precede the
    // row in the program); the row selects them by mask bit lane*3 + sum.
    // Only sums that may have fallen behind since they were last folded
    // (staleSums_) are visited, so consecutive rows over an unchanged window
    // skip the lazy-update walk.
    const RowSelect& sel = row_select(row);
    const uint32_t want = sel.mask[0] | sel.mask[1];
    uint32_t need = want & staleSums_;
    if (need)
        sumTableStale_ = true;   // a sum may grow below
    for (; need; need &= need - 1) {
        const unsigned k = (unsigned)__builtin_ctz(need);
        get_sum(k / kSums, k % kSums, count_);
        if (dead())
            return Siamese_Disabled;
    }
    staleSums_ &= ~want;
    if (sumTableStale_ || sumClipBytes_ != recoveryBytes) {
        // the 24 sums as the rows read them (rebuilt only after a change),
        // and the reference source bytes of each (clipped to the row)
        sumTableStale_ = false;
        sumTableVersion_ = Program::next_table_version();
        sumPresent_ = 0;
        sumClipBytes_ = recoveryBytes;
        for (unsigned k = 0; k < kRowSums; ++k) {
            const DevSum& d = lanes_[k / kSums].sum[k % kSums];
            WinEntry& t = sumTable_[k];
            t.src = d.buf.addr();
            t.len = d.bytes;
            t.column = 0;
            if (d.bytes > 0)
                sumPresent_ |= 1u << k;
            sumClip_[k] = std::min(d.bytes, recoveryBytes);
        }
    }
    const uint32_t mask[2] = {sel.mask[0] & sumPresent_, sel.mask[1] & sumPresent_};
    uint64_t opBytes = recoveryBytes; // final RX * product muladd
    for (unsigned h = 0; h < 2; ++h)
        for (uint32_t b = mask[h]; b; b &= b - 1)
            opBytes += sumClip_[__builtin_ctz(b)];
    sumEnd_ = count_;

    RowMeta m;
    m.sumCount = sumEnd_ - sumStart_ + sumErased_;
    m.ldpcCount = unacked();
    m.columnStart = sumColumnStart_;
    m.row = row;
    const unsigned footerBytes = write_footer(m, out.footer);

    // Sparse part (:1100-1144): ceil(n/16) PCG-chosen pairs, drawn on the
    // device, which also counts their reference source bytes
    const unsigned start = firstUnremoved_;
    const unsigned n = sumEnd_ - start;

    // Recovery = row sums ^ RX * product (:1232-1233) and its footer: one row
    // of the program's Siamese row batch (consecutive rows share the sums)
    cover(std::min(start, sumStart_), sumEnd_);
    prog_.rows_row(sumTable_, recovery_.addr(), recoveryBytes, 0, row_value(row), mask[0], mask[1], row,
                   n, start, count_, out.footer, footerBytes, sumTableVersion_);

    out.meta = m;
    out.footerBytes = footerBytes;
    out.buf = recovery_;
    out.bytes = recoveryBytes + footerBytes;
    stats_[SiameseEncoderStats_RecoveryCount]++;
    stats_[SiameseEncoderStats_RecoveryBytes] += out.bytes;
    lastRowSiamese_ = true;
    *opBytesOut = opBytes;
    return Siamese_Success;
}

SiameseResult EncoderCore::stats(uint64_t* out, unsigned count)
{
    if (count > SiameseEncoderStats_Count)
        count = SiameseEncoderStats_Count;
    uint64_t mem = recovery_.cap;
    for (auto& sw : subwindows_) {
        mem += sw->slab.buf.cap;
        if (sw->clean)
            continue;   // (no record written: no slot owns a buffer)
        for (EncSlot& s : sw->slot)
            if (!s.inSlab)
                mem += s.buf.cap;
    }
    for (Lane& l : lanes_)
        for (DevSum& s : l.sum)
            mem += s.buf.cap;
    stats_[SiameseEncoderStats_MemoryUsed] = mem;
    for (unsigned i = 0; i < count; ++i)
        out[i] = stats_[i];
    return Siamese_Success;
}

} // namespace sgpu
