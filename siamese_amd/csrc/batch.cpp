// batch.cpp -- siamese_gpu.h: the device-resident batch API.  Same control
// plane as the drop-in API; instances keep no host mirrors and never wait
// for the device until sgpu_flush().
#define SIAMESE_BUILDING
#include "../../include/siamese_gpu.h"

#include "backend.h"
#include "decoder.h"
#include "frames.h"
#include "encoder.h"
#include "engine.h"
#include "objpool.h"
#include "pool.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace sgpu;

namespace {

bool g_batchReady = false;

struct BatchEncoder
{
    EncoderCore core{Engine::global(), false};
};

struct BatchDecoder
{
    DecoderCore core{Engine::global(), false};
};

inline BatchEncoder* BE(SgpuEncoder e) { return reinterpret_cast<BatchEncoder*>(e); }
inline BatchDecoder* BD(SgpuDecoder d) { return reinterpret_cast<BatchDecoder*>(d); }
using Lock = std::lock_guard<std::mutex>;

// The routing sgpu_frames_recv_rows and sgpu_frames_recv_packed share: a
// record that passed its check (RowHead / PackedHead: the same fields), with
// its data at `data`, goes to its flow's decoder.
template <class Head>
SiameseResult route_head(const SgpuDecoder* decoders, unsigned decoderCount, const Head& h, uint64_t data,
                         unsigned* accepted)
{
    SiameseResult r = Siamese_InvalidInput;
    SgpuDecoder d = h.flow < decoderCount ? decoders[h.flow] : nullptr;
    // (a decoder with a device matrix job in flight takes no packets, as in sgpu_frames_recv)
    if (d && BD(d)->core.ge_pending())
        d = nullptr;
    if (d && h.type == kFrameOriginal) {
        SiameseOriginalPacket p;
        p.PacketNum = h.packetNum;
        p.Data = reinterpret_cast<const unsigned char*>((uintptr_t)data);
        p.DataBytes = h.dataBytes;
        r = BD(d)->core.add_original(p, data);
        ++*accepted;
    } else if (d) {
        RowMeta m;
        const uint8_t* tail = h.tail + 8 - h.tailBytes;
        const int footer = read_footer(tail, h.tailBytes, &m);
        if (footer > 0 && (unsigned)footer < h.dataBytes) {
            DeviceRecovery rec;
            rec.data = data;
            rec.bytes = h.dataBytes;
            rec.footer = h.tail + 8 - footer;
            rec.footerBytes = (unsigned)footer;
            rec.head = h.head;
            rec.producer = nullptr;   // ingested from the row, any alignment
            r = BD(d)->core.add_recovery_device(rec);
            ++*accepted;
        }
    }
    return r;
}

} // namespace

extern "C" {

SIAMESE_EXPORT int sgpu_init(int device)
{
    if (!gf_init())
        return Siamese_Disabled;
    Engine* eng = Engine::global();
    Lock lock(eng->mutex());
    const char* err = "unknown";
    if (!eng->init(device, &err)) {
        std::fprintf(stderr, "siamese_amd: initialisation failed: %s\n", err);
        return Siamese_Disabled;
    }
    g_batchReady = true;
    return Siamese_Success;
}

SIAMESE_EXPORT SgpuEncoder sgpu_encoder_create(void)
{
    if (!g_batchReady)
        return nullptr;
    // (storage recycled per thread: objpool.h RawPool)
    void* m = RawPool<BatchEncoder>::get();
    return m ? reinterpret_cast<SgpuEncoder>(new (m) BatchEncoder) : nullptr;
}

SIAMESE_EXPORT void sgpu_encoder_free(SgpuEncoder encoder)
{
    if (!encoder)
        return;
    BE(encoder)->~BatchEncoder();
    RawPool<BatchEncoder>::put(BE(encoder));
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_add(SgpuEncoder encoder, const void* deviceData, unsigned bytes,
                                              unsigned* packetNumOut)
{
    if (!encoder || !deviceData || bytes == 0 || bytes > SIAMESE_MAX_PACKET_BYTES)
        return Siamese_InvalidInput;
    SiameseOriginalPacket p;
    p.PacketNum = 0;
    p.Data = (const unsigned char*)deviceData;
    p.DataBytes = bytes;
    const SiameseResult r = BE(encoder)->core.add(p, (uint64_t)(uintptr_t)deviceData);
    if (packetNumOut)
        *packetNumOut = p.PacketNum;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_add_range(SgpuEncoder encoder, const void* deviceData, size_t stride,
                                                    const unsigned* bytes, unsigned fixedBytes, unsigned count,
                                                    unsigned* firstPacketNumOut, unsigned* addedOut)
{
    if (addedOut)
        *addedOut = 0;
    if (!encoder || (!deviceData && count) || stride > 0xffffffffu || (count > 1 && stride == 0))
        return Siamese_InvalidInput;
    unsigned first = 0, added = 0;
    const SiameseResult r = BE(encoder)->core.add_range((uint64_t)(uintptr_t)deviceData, (uint32_t)stride, bytes,
                                                        fixedBytes, count, &first, &added);
    if (firstPacketNumOut)
        *firstPacketNumOut = first;
    if (addedOut)
        *addedOut = added;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_remove_before(SgpuEncoder encoder, unsigned firstKept)
{
    if (!encoder || firstKept > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    BE(encoder)->core.remove_before(firstKept);
    return Siamese_Success;
}

SIAMESE_EXPORT SiameseResult sgpu_encode(SgpuEncoder encoder, SgpuRecoveryPacket* out)
{
    if (!encoder || !out)
        return Siamese_InvalidInput;
    EncoderCore& core = BE(encoder)->core;
    EncodeOut o;
    const SiameseResult r = core.encode(o);
    if (r != Siamese_Success) {
        out->DataBytes = 0;
        return r;
    }
    out->DeviceData = o.buf.ptr;
    out->DataBytes = o.bytes;
    out->FooterBytes = o.footerBytes;
    std::memcpy(out->Footer, o.footer, sizeof(out->Footer));
    std::memcpy(out->Head, o.head, sizeof(out->Head));
    out->Producer = &core.program();
    return Siamese_Success;
}

SIAMESE_EXPORT SiameseResult sgpu_encode_range(SgpuEncoder encoder, SgpuRecoveryPacket* out, unsigned count,
                                               unsigned* producedOut)
{
    if (producedOut)
        *producedOut = 0;
    if (!encoder || (!out && count) || !producedOut)
        return Siamese_InvalidInput;
    EncoderCore& core = BE(encoder)->core;
    // (EncodeOut is larger than the caller's records: encode in chunks)
    constexpr unsigned kChunk = 64;
    EncodeOut o[kChunk];
    SiameseResult r = Siamese_Success;
    unsigned done = 0;
    while (done < count && r == Siamese_Success) {
        const unsigned n = std::min(kChunk, count - done);
        unsigned made = 0;
        // (chunks after the first must keep the packets of the earlier ones:
        // one encode_range call per sgpu_encode_range, so chunking is by
        // hand below when count > kChunk)
        if (done == 0)
            r = core.encode_range(o, n, &made);
        else
            r = core.encode_range_more(o, n, &made);
        for (unsigned k = 0; k < made; ++k) {
            SgpuRecoveryPacket& p = out[done + k];
            p.DeviceData = o[k].buf.ptr;
            p.DataBytes = o[k].bytes;
            p.FooterBytes = o[k].footerBytes;
            std::memcpy(p.Footer, o[k].footer, sizeof(p.Footer));
            std::memcpy(p.Head, o[k].head, sizeof(p.Head));
            p.Producer = &core.program();
        }
        done += made;
        if (made < n && r == Siamese_Success)
            break;
    }
    if (r != Siamese_Success && done < count)
        out[done].DataBytes = 0;
    *producedOut = done;
    return r;
}

namespace {

/// The row arguments the two framing calls share (siamese_gpu.h).
bool frame_rows_ok(unsigned count, uint64_t dst, size_t stride, uint64_t lens)
{
    return !((!dst || !lens) && count) && (dst & 15u) == 0 && stride != 0 && (stride & 15u) == 0 &&
           (uint64_t)stride <= (1ull << 32) && (lens & 3u) == 0;
}

} // namespace

SIAMESE_EXPORT SiameseResult sgpu_encoder_deliver_range(SgpuEncoder encoder, unsigned firstPacketNum, unsigned count,
                                                        unsigned flow, void* deviceDst, size_t stride,
                                                        unsigned* deviceLens, SiameseResult* results,
                                                        unsigned* queuedOut)
{
    if (queuedOut)
        *queuedOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    if (!encoder || !frame_rows_ok(count, dst, stride, lens) || (flow > kFrameMaxFlow && flow != SGPU_FRAME_NONE) ||
        firstPacketNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    static_assert(EncoderCore::kFrameNone == SGPU_FRAME_NONE, "SGPU_FRAME_NONE");
    unsigned queued = 0;
    const SiameseResult r = BE(encoder)->core.deliver_range(firstPacketNum, count, flow, dst, (uint64_t)stride, lens,
                                                            results, &queued);
    if (queuedOut)
        *queuedOut = queued;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_frames_deliver_recovery(unsigned count, const SgpuRecoveryPacket* packets,
                                                          const unsigned* flows, void* deviceDst, size_t stride,
                                                          unsigned* deviceLens, unsigned* queuedOut)
{
    if (queuedOut)
        *queuedOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    if ((!packets && count) || !frame_rows_ok(count, dst, stride, lens))
        return Siamese_InvalidInput;
    // every packet is checked before any is queued
    for (unsigned k = 0; k < count; ++k) {
        const SgpuRecoveryPacket& p = packets[k];
        // (DataBytes as sgpu_frames_send takes them)
        if (!p.DeviceData || !p.Producer || p.DataBytes == 0 || p.DataBytes > SIAMESE_MAX_PACKET_BYTES ||
            (flows && flows[k] > kFrameMaxFlow && flows[k] != SGPU_FRAME_NONE))
            return Siamese_InvalidInput;
        const bool framed = flows && flows[k] != SGPU_FRAME_NONE;
        if ((uint64_t)(framed ? frame_header_bytes(kFrameRecovery, p.DataBytes) : 0) + p.DataBytes > stride)
            return Siamese_InvalidInput;
    }
    if (!g_batchReady || Engine::global()->failed())
        return Siamese_Disabled;
    for (unsigned k = 0; k < count; ++k) {
        const SgpuRecoveryPacket& p = packets[k];
        uint8_t hdr[kFrameMaxHeader] = {};
        unsigned h = 0;
        if (flows && flows[k] != SGPU_FRAME_NONE)
            h = frame_write_header(kFrameRecovery, flows[k], 0, p.DataBytes, hdr);
        // (on the producing encoder's program, as sgpu_decoder_add_recovery's copy)
        reinterpret_cast<Program*>(p.Producer)->frame((uint64_t)(uintptr_t)p.DeviceData, p.DataBytes, hdr, h,
                                                      dst + (uint64_t)k * stride, lens + (uint64_t)k * 4,
                                                      (uint64_t)stride);
    }
    if (queuedOut)
        *queuedOut = count;
    return Siamese_Success;
}

SIAMESE_EXPORT SgpuDecoder sgpu_decoder_create(void)
{
    if (!g_batchReady)
        return nullptr;
    void* m = RawPool<BatchDecoder>::get();
    return m ? reinterpret_cast<SgpuDecoder>(new (m) BatchDecoder) : nullptr;
}

SIAMESE_EXPORT void sgpu_decoder_free(SgpuDecoder decoder)
{
    if (!decoder)
        return;
    BD(decoder)->~BatchDecoder();
    RawPool<BatchDecoder>::put(BD(decoder));
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_add_original(SgpuDecoder decoder, unsigned packetNum,
                                                       const void* deviceData, unsigned bytes)
{
    if (!decoder || BD(decoder)->core.ge_pending() || !deviceData || bytes == 0 || bytes > SIAMESE_MAX_PACKET_BYTES ||
        packetNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    SiameseOriginalPacket p;
    p.PacketNum = packetNum;
    p.Data = (const unsigned char*)deviceData;
    p.DataBytes = bytes;
    return BD(decoder)->core.add_original(p, (uint64_t)(uintptr_t)deviceData);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_add_original_range(SgpuDecoder decoder, unsigned firstPacketNum,
                                                             const void* deviceData, size_t stride,
                                                             const unsigned* bytes, unsigned fixedBytes,
                                                             unsigned count, SiameseResult* results,
                                                             unsigned* callsOut)
{
    if (callsOut)
        *callsOut = 0;
    if (!decoder || BD(decoder)->core.ge_pending() || (!deviceData && count) || firstPacketNum > SIAMESE_PACKET_NUM_MAX || stride > 0xffffffffu ||
        (count > 1 && stride == 0))
        return Siamese_InvalidInput;
    unsigned calls = 0;
    const SiameseResult r = BD(decoder)->core.add_original_range(firstPacketNum, (uint64_t)(uintptr_t)deviceData,
                                                                 (uint32_t)stride, bytes, fixedBytes, count, results,
                                                                 &calls);
    if (callsOut)
        *callsOut = calls;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_add_recovery(SgpuDecoder decoder, const SgpuRecoveryPacket* packet)
{
    if (!decoder || BD(decoder)->core.ge_pending() || !packet || !packet->DeviceData || packet->DataBytes == 0 ||
        packet->FooterBytes == 0 || packet->FooterBytes > 8 || packet->FooterBytes >= packet->DataBytes)
        return Siamese_InvalidInput;
    DeviceRecovery r;
    r.data = (uint64_t)(uintptr_t)packet->DeviceData;
    r.bytes = packet->DataBytes;
    r.footer = packet->Footer;
    r.footerBytes = packet->FooterBytes;
    r.head = packet->Head;
    r.producer = reinterpret_cast<Program*>(packet->Producer);
    return BD(decoder)->core.add_recovery_device(r);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_is_ready(SgpuDecoder decoder)
{
    if (!decoder || BD(decoder)->core.ge_pending())
        return Siamese_InvalidInput;
    return BD(decoder)->core.is_ready();
}

SIAMESE_EXPORT SiameseResult sgpu_decode(SgpuDecoder decoder, SiameseOriginalPacket** packetsOut,
                                         unsigned* countOut)
{
    if (!decoder || BD(decoder)->core.ge_pending() || (!packetsOut != !countOut))
        return Siamese_InvalidInput;
    return BD(decoder)->core.decode(packetsOut, countOut);
}

SIAMESE_EXPORT SiameseResult sgpu_decode_device(SgpuDecoder decoder, SiameseOriginalPacket** packetsOut,
                                                unsigned* countOut)
{
    if (!decoder || (!packetsOut != !countOut))
        return Siamese_InvalidInput;
    return BD(decoder)->core.decode_device(packetsOut, countOut);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_get(SgpuDecoder decoder, SiameseOriginalPacket* packet)
{
    if (!decoder || BD(decoder)->core.ge_pending() || !packet || packet->PacketNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    return BD(decoder)->core.get(*packet);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_get_range(SgpuDecoder decoder, unsigned firstPacketNum, unsigned count,
                                                    SiameseOriginalPacket* packets, unsigned* gotOut)
{
    if (gotOut)
        *gotOut = 0;
    if (!decoder || BD(decoder)->core.ge_pending() || (!packets && count) || !gotOut || firstPacketNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    return BD(decoder)->core.get_range(firstPacketNum, count, packets, gotOut);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_deliver_range(SgpuDecoder decoder, unsigned firstPacketNum, unsigned count,
                                                        void* deviceDst, size_t stride, unsigned* deviceLens,
                                                        SiameseResult* results, unsigned* queuedOut)
{
    if (queuedOut)
        *queuedOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    if (!decoder || BD(decoder)->core.ge_pending() || ((!deviceDst || !deviceLens) && count) || (dst & 15u) ||
        stride == 0 || (stride & 15u) || (uint64_t)stride > (1ull << 32) || (lens & 3u) ||
        firstPacketNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    unsigned queued = 0;
    const SiameseResult r =
        BD(decoder)->core.deliver_range(firstPacketNum, count, dst, (uint64_t)stride, lens, results, &queued);
    if (queuedOut)
        *queuedOut = queued;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_deliver_frames(SgpuDecoder decoder, unsigned flow, unsigned firstPacketNum,
                                                         unsigned count, void* deviceDst, size_t stride,
                                                         unsigned* deviceLens, SiameseResult* results,
                                                         unsigned* queuedOut)
{
    if (queuedOut)
        *queuedOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    // (SGPU_FRAME_NONE is above kFrameMaxFlow: the bare form is sgpu_decoder_deliver_range)
    if (!decoder || BD(decoder)->core.ge_pending() || !frame_rows_ok(count, dst, stride, lens) ||
        flow > kFrameMaxFlow || firstPacketNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    unsigned queued = 0;
    const SiameseResult r = BD(decoder)->core.deliver_frames(firstPacketNum, count, flow, dst, (uint64_t)stride,
                                                             lens, results, &queued);
    if (queuedOut)
        *queuedOut = queued;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_pack_frames(SgpuDecoder decoder, unsigned flow, unsigned firstPacketNum,
                                                      unsigned count, void* deviceDst, size_t stride, unsigned maxRows,
                                                      unsigned* deviceLens, unsigned* deviceInfo,
                                                      SiameseResult* results, unsigned* queuedOut)
{
    if (queuedOut)
        *queuedOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    const uint64_t info = (uint64_t)(uintptr_t)deviceInfo;
    // (frame_rows_ok on maxRows: the rows and length words are the caller's whatever the packet count)
    if (!decoder || BD(decoder)->core.ge_pending() || !frame_rows_ok(maxRows, dst, stride, lens) || !info ||
        (info & 15u) != 0 || flow > kFrameMaxFlow || firstPacketNum > SIAMESE_PACKET_NUM_MAX || count > kPackMaxItems)
        return Siamese_InvalidInput;
    unsigned queued = 0;
    const SiameseResult r = BD(decoder)->core.pack_frames(firstPacketNum, count, flow, dst, (uint64_t)stride, maxRows,
                                                          lens, info, results, &queued);
    if (queuedOut)
        *queuedOut = queued;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_deliver_stream(SgpuDecoder decoder, unsigned firstPacketNum, unsigned count,
                                                         void* deviceDst, size_t capacity, unsigned* deviceOffsets,
                                                         unsigned* deviceInfo, SiameseResult* results,
                                                         unsigned* queuedOut)
{
    if (queuedOut)
        *queuedOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, offsets = (uint64_t)(uintptr_t)deviceOffsets;
    const uint64_t info = (uint64_t)(uintptr_t)deviceInfo;
    // (deviceDst has any alignment: a receiver appends at its write cursor)
    if (!decoder || !queuedOut || BD(decoder)->core.ge_pending() || !offsets || (offsets & 3u) != 0 || !info ||
        (info & 15u) != 0 || (!deviceDst && capacity) || (uint64_t)capacity > 0xffffffffull ||
        count > kConcatMaxItems || firstPacketNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    unsigned queued = 0;
    const SiameseResult r = BD(decoder)->core.deliver_stream(firstPacketNum, count, dst, (uint32_t)capacity, offsets,
                                                             info, results, &queued);
    *queuedOut = queued;
    return r;
}

SIAMESE_EXPORT SiameseResult sgpu_decode_deferred(SgpuDecoder decoder, SiameseOriginalPacket* out,
                                                  unsigned capacity, unsigned* countOut)
{
    if (!decoder || BD(decoder)->core.ge_pending() || !out || !countOut)
        return Siamese_InvalidInput;
    return BD(decoder)->core.decode_deferred(out, capacity, countOut);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_get_deferred(SgpuDecoder decoder, SiameseOriginalPacket* packet)
{
    if (!decoder || BD(decoder)->core.ge_pending() || !packet || packet->PacketNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    return BD(decoder)->core.get_deferred(*packet);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_has(SgpuDecoder decoder, unsigned packetNum)
{
    if (!decoder || BD(decoder)->core.ge_pending() || packetNum > SIAMESE_PACKET_NUM_MAX)
        return Siamese_InvalidInput;
    return BD(decoder)->core.has(packetNum) ? Siamese_Success : Siamese_NeedMoreData;
}

SIAMESE_EXPORT int sgpu_flush(void)
{
    Engine* eng = Engine::global();
    Lock lock(eng->mutex());
    return eng->flush_and_sync() ? 0 : -1;
}

SIAMESE_EXPORT int sgpu_submit(void)
{
    Engine* eng = Engine::global();
    Lock lock(eng->mutex());
    return eng->flush() ? 0 : -1;
}

SIAMESE_EXPORT long long sgpu_enqueue(void)
{
    Engine* eng = Engine::global();
    Lock lock(eng->mutex());
    const uint64_t t = eng->enqueue();
    return eng->failed() ? -1 : (long long)t;
}

SIAMESE_EXPORT int sgpu_wait(long long ticket)
{
    // no engine lock: other threads keep driving instances meanwhile
    if (ticket < 0)
        return -1;
    return Engine::global()->wait((uint64_t)ticket) ? 0 : -1;
}

SIAMESE_EXPORT int sgpu_query(long long ticket)
{
    Engine* eng = Engine::global();
    if (ticket < 0 || eng->failed())
        return -1;
    return eng->done((uint64_t)ticket) ? 1 : 0;
}

SIAMESE_EXPORT void sgpu_parallel_for(unsigned count, void (*fn)(void* ctx, unsigned index), void* ctx)
{
    if (!fn)
        return;
    Engine::global()->pool().run(count, [&](size_t i) { fn(ctx, (unsigned)i); });
}

SIAMESE_EXPORT void* sgpu_device_alloc(size_t bytes)
{
    if (!g_batchReady)
        return nullptr;
    Lock lock(Engine::global()->mutex());
    return be_dev_alloc(bytes);
}

SIAMESE_EXPORT void sgpu_device_free(void* p)
{
    Lock lock(Engine::global()->mutex());
    be_dev_free(p);
}

SIAMESE_EXPORT void* sgpu_host_alloc(size_t bytes)
{
    if (!g_batchReady)
        return nullptr;
    Lock lock(Engine::global()->mutex());
    return be_host_alloc(bytes);
}

SIAMESE_EXPORT void sgpu_host_free(void* p)
{
    Lock lock(Engine::global()->mutex());
    be_host_free(p);
}

SIAMESE_EXPORT int sgpu_h2d(void* deviceDst, const void* hostSrc, size_t bytes)
{
    Engine* eng = Engine::global();
    Lock lock(eng->mutex());
    if (!eng->sync())
        return -1;
    be_h2d(deviceDst, hostSrc, bytes);
    return be_sync() ? 0 : -1;
}

SIAMESE_EXPORT int sgpu_gather(unsigned count, const void* const* deviceSrcs, const unsigned* bytes,
                               void* hostOut)
{
    Engine* eng = Engine::global();
    Lock lock(eng->mutex());
    return eng->gather(count, deviceSrcs, bytes, hostOut) ? 0 : -1;
}

SIAMESE_EXPORT int sgpu_h2d_async(void* deviceDst, const void* hostSrc, size_t bytes)
{
    if (!g_batchReady)
        return -1;
    return Engine::global()->stage_in(deviceDst, hostSrc, bytes) ? 0 : -1;
}

SIAMESE_EXPORT int sgpu_gather_completed(unsigned count, const void* const* deviceSrcs, const unsigned* bytes,
                                         void* pinnedOut)
{
    if (!g_batchReady)
        return -1;
    return Engine::global()->gather_completed(count, deviceSrcs, bytes, pinnedOut) ? 0 : -1;
}

SIAMESE_EXPORT long long sgpu_gather_async(unsigned count, const void* const* deviceSrcs, const unsigned* bytes,
                                           void* pinnedOut)
{
    if (!g_batchReady)
        return -1;
    return (long long)Engine::global()->gather_async(count, deviceSrcs, bytes, pinnedOut);
}

SIAMESE_EXPORT int sgpu_gather_wait(long long ticket)
{
    if (!g_batchReady)
        return -1;
    return Engine::global()->gather_wait((int64_t)ticket) ? 0 : -1;
}

SIAMESE_EXPORT unsigned sgpu_frame_header_bytes(unsigned type, unsigned dataBytes)
{
    if (type > SGPU_FRAME_RECOVERY)
        return 0;
    return frame_header_bytes(type, dataBytes);
}

SIAMESE_EXPORT unsigned sgpu_frame_write_header(unsigned type, unsigned flow, unsigned packetNum,
                                                unsigned dataBytes, void* out)
{
    if (!out || type > SGPU_FRAME_RECOVERY || flow > kFrameMaxFlow || packetNum > SIAMESE_PACKET_NUM_MAX ||
        dataBytes == 0 || dataBytes > SIAMESE_MAX_PACKET_BYTES)
        return 0;
    return frame_write_header(type, flow, packetNum, dataBytes, static_cast<uint8_t*>(out));
}

SIAMESE_EXPORT SiameseResult sgpu_frames_parse(const void* frames, size_t bytes, SgpuFrame* out,
                                               unsigned maxFrames, unsigned* countOut)
{
    if (!frames || !out || !countOut)
        return Siamese_InvalidInput;
    *countOut = 0;
    if (bytes > UINT32_MAX)   // (frame offsets are 32-bit)
        return Siamese_InvalidInput;
    static_assert(sizeof(SgpuFrame) == sizeof(FrameInfo), "SgpuFrame layout");
    size_t consumed = 0, bad = 0;
    const long n = frames_parse(static_cast<const uint8_t*>(frames), bytes, reinterpret_cast<FrameInfo*>(out),
                                maxFrames, &consumed, &bad);
    // (the frames before a malformed one are returned with InvalidInput)
    *countOut = (unsigned)n;
    return consumed == bytes && bad == kNoBadFrame ? Siamese_Success : Siamese_InvalidInput;
}

SIAMESE_EXPORT SiameseResult sgpu_frames_recv(const SgpuDecoder* decoders, unsigned decoderCount,
                                              const void* hostFrames, const void* deviceFrames, size_t bytes,
                                              SiameseResult* results, unsigned maxFrames, unsigned* countOut)
{
    if (!decoders || !hostFrames || !deviceFrames || !countOut)
        return Siamese_InvalidInput;
    *countOut = 0;
    if (bytes > UINT32_MAX)   // (frame offsets are 32-bit)
        return Siamese_InvalidInput;
    const uint8_t* host = static_cast<const uint8_t*>(hostFrames);
    const uint64_t dev = (uint64_t)(uintptr_t)deviceFrames;
    // parse in blocks: the headers of a whole ring in one pass, then the calls
    FrameInfo fi[256];
    size_t at = 0;
    unsigned done = 0;
    SiameseResult status = Siamese_Success;
    bool malformed = false;
    while (at < bytes && done < maxFrames && !malformed) {
        size_t consumed = 0, bad = 0;
        const size_t want = std::min<size_t>(256, maxFrames - done);
        const long n = frames_parse(host + at, bytes - at, fi, want, &consumed, &bad);
        // every well-formed frame before a malformed one is still delivered;
        // the ring is not read past the malformed frame (its length cannot be
        // trusted to find the next one)
        malformed = bad != kNoBadFrame;
        for (long k = 0; k < n; ++k) {
            const FrameInfo& f = fi[k];
            const size_t off = at + f.offset;
            SiameseResult r = Siamese_InvalidInput;
            SgpuDecoder d = f.flow < decoderCount ? decoders[f.flow] : nullptr;
            // (a decoder with a device matrix job in flight takes no packets:
            // the job was built from its current window, like every other
            // sgpu_decoder_* call it answers InvalidInput until decode_device
            // has finished the job)
            if (d && BD(d)->core.ge_pending())
                d = nullptr;
            if (d && f.type == kFrameOriginal) {
                if (f.bytes <= SIAMESE_MAX_PACKET_BYTES && f.packetNum <= SIAMESE_PACKET_NUM_MAX) {
                    SiameseOriginalPacket p;
                    p.PacketNum = f.packetNum;
                    p.Data = reinterpret_cast<const unsigned char*>((uintptr_t)(dev + off));
                    p.DataBytes = f.bytes;
                    r = BD(d)->core.add_original(p, dev + off);
                }
            } else if (d && f.type == kFrameRecovery) {
                RowMeta m;
                const int footer = read_footer(host + off, f.bytes, &m);
                if (footer > 0 && (unsigned)footer < f.bytes) {
                    DeviceRecovery rec;
                    rec.data = dev + off;
                    rec.bytes = f.bytes;
                    rec.footer = host + off + f.bytes - footer;
                    rec.footerBytes = (unsigned)footer;
                    rec.head = host + off;
                    rec.producer = nullptr;   // staged: ingested from the device copy
                    r = BD(d)->core.add_recovery_device(rec);
                }
            }
            if (results)
                results[done] = r;
            if (r != Siamese_Success && status == Siamese_Success)
                status = r;
            ++done;
        }
        at += consumed;
        if (n == 0)
            break;
    }
    *countOut = done;
    return at >= bytes && !malformed ? status : Siamese_InvalidInput;
}

namespace {
static_assert(sizeof(SgpuRowHead) == sizeof(RowHead) && offsetof(SgpuRowHead, Status) == offsetof(RowHead, status) &&
                  offsetof(SgpuRowHead, Flow) == offsetof(RowHead, flow) &&
                  offsetof(SgpuRowHead, DataBytes) == offsetof(RowHead, dataBytes) &&
                  offsetof(SgpuRowHead, Head) == offsetof(RowHead, head) &&
                  offsetof(SgpuRowHead, Tail) == offsetof(RowHead, tail),
              "SgpuRowHead layout");
static_assert(SGPU_ROW_EMPTY == kRowEmpty && SGPU_ROW_OK == kRowOk && SGPU_ROW_MALFORMED == kRowMalformed,
              "SgpuRowHead status values");

// the row arguments sgpu_frames_scan_rows and sgpu_frames_recv_rows share
inline bool rows_ok(const void* deviceRows, size_t stride, unsigned count)
{
    if (stride == 0 || (stride & 15) || stride > ((uint64_t)1 << 32))
        return false;
    if ((uintptr_t)deviceRows & 15)
        return false;
    return deviceRows || count == 0;
}

static_assert(sizeof(SgpuPackedHead) == sizeof(PackedHead) && offsetof(SgpuPackedHead, Offset) == offsetof(PackedHead, offset) &&
                  offsetof(SgpuPackedHead, Status) == offsetof(PackedHead, status) &&
                  offsetof(SgpuPackedHead, Flow) == offsetof(PackedHead, flow) &&
                  offsetof(SgpuPackedHead, DataBytes) == offsetof(PackedHead, dataBytes) &&
                  offsetof(SgpuPackedHead, Head) == offsetof(PackedHead, head) &&
                  offsetof(SgpuPackedHead, Tail) == offsetof(PackedHead, tail),
              "SgpuPackedHead layout");
static_assert(SGPU_PACKED_MORE == kPackedMore && SGPU_PACKED_MALFORMED == kPackedMalformed &&
                  SGPU_PACKED_COUNT(0xffffffffu) == kPackedCountMask,
              "SgpuPackedHead row word");
} // namespace

SIAMESE_EXPORT long long sgpu_frames_scan_rows(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                               unsigned count, SgpuRowHead* pinnedOut)
{
    if (!g_batchReady || !rows_ok(deviceRows, stride, count) || ((uintptr_t)deviceLens & 3) ||
        ((uintptr_t)pinnedOut & 15) || (!pinnedOut && count > 0))
        return -1;
    return (long long)Engine::global()->scan_rows_async(deviceRows, stride, deviceLens, count, pinnedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_frames_recv_rows(const SgpuDecoder* decoders, unsigned decoderCount,
                                                   const SgpuRowHead* heads, const void* deviceRows, size_t stride,
                                                   unsigned count, SiameseResult* results, unsigned* acceptedOut)
{
    if (!acceptedOut)
        return Siamese_InvalidInput;
    *acceptedOut = 0;
    if (!rows_ok(deviceRows, stride, count) || ((!decoders || !heads) && count > 0) || ((uintptr_t)heads & 3))
        return Siamese_InvalidInput;
    const uint64_t dev = (uint64_t)(uintptr_t)deviceRows;
    unsigned accepted = 0;
    SiameseResult status = Siamese_Success;
    for (unsigned k = 0; k < count; ++k) {
        // (the records are the caller's memory: each is copied, checked and only then used)
        RowHead h;
        std::memcpy(&h, &heads[k], sizeof(h));
        SiameseResult r = Siamese_InvalidInput;
        if (h.status == kRowEmpty)
            r = Siamese_NeedMoreData;
        else if (row_head_valid(h, stride))
            r = route_head(decoders, decoderCount, h, dev + (uint64_t)k * stride + h.headerBytes, &accepted);
        if (results)
            results[k] = r;
        if (r != Siamese_Success && r != Siamese_NeedMoreData && status == Siamese_Success)
            status = r;
    }
    *acceptedOut = accepted;
    return status;
}

SIAMESE_EXPORT size_t sgpu_frames_packed_bytes(unsigned count, unsigned maxFrames)
{
    return maxFrames >= 1 && maxFrames <= kPackedMaxFrames ? (size_t)packed_bytes(count, maxFrames) : 0;
}

SIAMESE_EXPORT long long sgpu_frames_scan_packed(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                                 unsigned count, unsigned maxFrames, void* pinnedOut)
{
    if (!g_batchReady || !rows_ok(deviceRows, stride, count) || ((uintptr_t)deviceLens & 3) ||
        ((uintptr_t)pinnedOut & 15) || (!pinnedOut && count > 0) || maxFrames < 1 || maxFrames > kPackedMaxFrames ||
        packed_bytes(count, maxFrames) > ((uint64_t)1 << 32))
        return -1;
    return (long long)Engine::global()->walk_rows_async(deviceRows, stride, deviceLens, count, maxFrames, pinnedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_frames_recv_packed(const SgpuDecoder* decoders, unsigned decoderCount,
                                                     const void* heads, unsigned maxFrames, const void* deviceRows,
                                                     size_t stride, unsigned count, SiameseResult* results,
                                                     unsigned* acceptedOut)
{
    if (!acceptedOut)
        return Siamese_InvalidInput;
    *acceptedOut = 0;
    if (!rows_ok(deviceRows, stride, count) || ((!decoders || !heads) && count > 0) || ((uintptr_t)heads & 3) ||
        maxFrames < 1 || maxFrames > kPackedMaxFrames)
        return Siamese_InvalidInput;
    const uint64_t dev = (uint64_t)(uintptr_t)deviceRows;
    const uint8_t* recs = static_cast<const uint8_t*>(heads);
    const uint8_t* words = recs + (size_t)count * maxFrames * sizeof(PackedHead);
    unsigned accepted = 0;
    SiameseResult status = Siamese_Success;
    for (unsigned k = 0; k < count; ++k) {
        // (the words and records are the caller's memory: each is copied, checked and only then used)
        uint32_t word;
        std::memcpy(&word, words + (size_t)k * 4, 4);
        SiameseResult* res = results ? results + (size_t)k * maxFrames : nullptr;
        for (unsigned j = 0; res && j < maxFrames; ++j)
            res[j] = Siamese_NeedMoreData;
        unsigned n = word & kPackedCountMask;
        bool malformed = (word & kPackedMalformed) != 0;
        if (n > maxFrames) {   // (no scan writes such a word: none of the row's records is used)
            n = 0;
            malformed = true;
        }
        for (unsigned j = 0; j < n; ++j) {
            PackedHead h;
            std::memcpy(&h, recs + ((size_t)k * maxFrames + j) * sizeof(h), sizeof(h));
            SiameseResult r = Siamese_InvalidInput;
            if (packed_head_valid(h, stride))
                r = route_head(decoders, decoderCount, h, dev + (uint64_t)k * stride + h.offset + h.headerBytes,
                               &accepted);
            if (res)
                res[j] = r;
            if (r != Siamese_Success && r != Siamese_NeedMoreData && status == Siamese_Success)
                status = r;
        }
        if (malformed) {   // the frame the walk stopped at: the slot after the row's last record, if there is one
            if (res && n < maxFrames)
                res[n] = Siamese_InvalidInput;
            if (status == Siamese_Success)
                status = Siamese_InvalidInput;
        }
    }
    *acceptedOut = accepted;
    return status;
}

namespace {
// the sizes sgpu_frames_dense_bytes, sgpu_frames_scan_dense and sgpu_frames_recv_dense share
inline bool dense_ok(unsigned count, unsigned maxFrames, unsigned maxRecords)
{
    return maxFrames >= 1 && maxFrames <= kPackedMaxFrames && maxRecords >= maxFrames &&
           (uint64_t)maxRecords <= (uint64_t)count * maxFrames;
}
} // namespace

SIAMESE_EXPORT size_t sgpu_frames_dense_bytes(unsigned count, unsigned maxRecords)
{
    // (what no maxFrames allows: fewer than one record, more than 256 per row)
    return maxRecords >= 1 && (uint64_t)maxRecords <= (uint64_t)count * kPackedMaxFrames
               ? (size_t)dense_bytes(count, maxRecords)
               : 0;
}

SIAMESE_EXPORT size_t sgpu_frames_dense_records(unsigned count)
{
    return (size_t)dense_records_offset(count);
}

SIAMESE_EXPORT long long sgpu_frames_scan_dense(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                                unsigned count, unsigned maxFrames, unsigned maxRecords,
                                                void* pinnedOut)
{
    if (!g_batchReady || !rows_ok(deviceRows, stride, count) || ((uintptr_t)deviceLens & 3) ||
        ((uintptr_t)pinnedOut & 15) || (!pinnedOut && count > 0) || maxFrames < 1 || maxFrames > kPackedMaxFrames ||
        packed_bytes(count, maxFrames) > ((uint64_t)1 << 32))
        return -1;
    // (count == 0 admits no maxRecords >= maxFrames: its ticket is complete and nothing is written)
    if (count > 0 && (!dense_ok(count, maxFrames, maxRecords) || dense_bytes(count, maxRecords) >= ((uint64_t)1 << 32)))
        return -1;
    return (long long)Engine::global()->dense_rows_async(deviceRows, stride, deviceLens, count, maxFrames,
                                                         count ? maxRecords : 0, pinnedOut);
}

namespace {
// sgpu_frames_recv_dense and, with the next words behind the dense part (streams) and consumedOut,
// sgpu_frames_recv_streams
SiameseResult recv_dense_rows(const SgpuDecoder* decoders, unsigned decoderCount, const void* heads,
                              unsigned maxFrames, unsigned maxRecords, const void* deviceRows, size_t stride,
                              unsigned count, SiameseResult* results, bool streams, unsigned* consumedOut,
                              unsigned* rowsOut, unsigned* acceptedOut)
{
    if (rowsOut)
        *rowsOut = 0;
    if (!acceptedOut)
        return Siamese_InvalidInput;
    *acceptedOut = 0;
    if (!rowsOut || !rows_ok(deviceRows, stride, count) || ((!decoders || !heads) && count > 0) ||
        ((uintptr_t)heads & 3) || maxFrames < 1 || maxFrames > kPackedMaxFrames ||
        (count > 0 && !dense_ok(count, maxFrames, maxRecords)) || (streams && !consumedOut && count > 0))
        return Siamese_InvalidInput;
    if (count == 0)
        return Siamese_Success;
    for (unsigned i = 0; results && i < maxRecords; ++i)
        results[i] = Siamese_NeedMoreData;
    // (the output is the caller's memory: every word and record is copied, checked and only then used)
    const uint64_t dev = (uint64_t)(uintptr_t)deviceRows;
    const uint8_t* base = static_cast<const uint8_t*>(heads);
    const uint8_t* words = base + 16;
    const uint8_t* starts = words + (size_t)count * 4;
    const uint8_t* recs = base + (size_t)dense_records_offset(count);
    const uint8_t* nextWords = streams ? base + (size_t)streams_next_offset(count, maxRecords) : nullptr;
    uint32_t info[4];
    std::memcpy(info, base, sizeof(info));
    const uint32_t W = info[1], c = info[2];
    if (c > count || W > maxRecords)
        return Siamese_InvalidInput;
    unsigned accepted = 0;
    SiameseResult status = Siamese_Success;
    uint32_t at = 0;   // start[k], checked
    std::memcpy(&at, starts, 4);
    bool forged = at != 0;
    unsigned k = 0;
    for (; !forged && k < c; ++k) {
        uint32_t word, next;
        std::memcpy(&word, words + (size_t)k * 4, 4);
        std::memcpy(&next, starts + (size_t)(k + 1) * 4, 4);
        unsigned n = word & kPackedCountMask;
        bool malformed = (word & kPackedMalformed) != 0;
        const unsigned span = n < maxFrames ? n : maxFrames;
        // the row's records are [at, next): non-decreasing, as many as its word says, and before W
        if (next < at || next - at != span || next > W) {
            forged = true;
            break;
        }
        if (n > maxFrames) {   // (no scan writes such a word: none of the row's records is used)
            n = 0;
            malformed = true;
        }
        uint32_t resume = 0;
        if (nextWords) {
            // where the row's next scan starts: within the row, and not before the end of its last record
            std::memcpy(&resume, nextWords + (size_t)k * 4, 4);
            uint64_t least = 0;
            if (n > 0) {
                PackedHead h;
                std::memcpy(&h, recs + ((size_t)at + n - 1) * sizeof(h), sizeof(h));
                least = (uint64_t)h.offset + h.headerBytes + h.dataBytes;
            }
            if (resume > stride || resume < least) {
                forged = true;
                break;
            }
        }
        for (unsigned j = 0; j < n; ++j) {
            PackedHead h;
            std::memcpy(&h, recs + ((size_t)at + j) * sizeof(h), sizeof(h));
            SiameseResult r = Siamese_InvalidInput;
            if (packed_head_valid(h, stride))
                r = route_head(decoders, decoderCount, h, dev + (uint64_t)k * stride + h.offset + h.headerBytes,
                               &accepted);
            if (results)
                results[at + j] = r;
            if (r != Siamese_Success && r != Siamese_NeedMoreData && status == Siamese_Success)
                status = r;
        }
        if (malformed && status == Siamese_Success)   // (the frame the walk stopped at has no slot here)
            status = Siamese_InvalidInput;
        if (nextWords)
            consumedOut[k] = resume;
        at = next;
    }
    if (!forged && at != W)
        forged = true;
    *rowsOut = k;   // c, unless the table stopped the routing before it
    *acceptedOut = accepted;
    return forged ? Siamese_InvalidInput : status;
}
} // namespace

SIAMESE_EXPORT SiameseResult sgpu_frames_recv_dense(const SgpuDecoder* decoders, unsigned decoderCount,
                                                    const void* heads, unsigned maxFrames, unsigned maxRecords,
                                                    const void* deviceRows, size_t stride, unsigned count,
                                                    SiameseResult* results, unsigned* rowsOut,
                                                    unsigned* acceptedOut)
{
    return recv_dense_rows(decoders, decoderCount, heads, maxFrames, maxRecords, deviceRows, stride, count, results,
                           false, nullptr, rowsOut, acceptedOut);
}

static_assert(SGPU_STREAM_PARTIAL == kStreamPartial && !(SGPU_STREAM_PARTIAL & (kPackedCountMask | kPackedMore |
                                                                                 kPackedMalformed)),
              "the stream scan's row word");

SIAMESE_EXPORT size_t sgpu_frames_streams_bytes(unsigned count, unsigned maxRecords)
{
    return sgpu_frames_dense_bytes(count, maxRecords) ? (size_t)streams_bytes(count, maxRecords) : 0;
}

SIAMESE_EXPORT size_t sgpu_frames_streams_next(unsigned count, unsigned maxRecords)
{
    return sgpu_frames_dense_bytes(count, maxRecords) ? (size_t)streams_next_offset(count, maxRecords) : 0;
}

SIAMESE_EXPORT long long sgpu_frames_scan_streams(const void* deviceRows, size_t stride, const unsigned* deviceStarts,
                                                  const unsigned* deviceEnds, unsigned count, unsigned maxFrames,
                                                  unsigned maxRecords, void* pinnedOut)
{
    if (!g_batchReady || !rows_ok(deviceRows, stride, count) || ((uintptr_t)deviceStarts & 3) ||
        ((uintptr_t)deviceEnds & 3) || ((uintptr_t)pinnedOut & 15) || (!pinnedOut && count > 0) || maxFrames < 1 ||
        maxFrames > kPackedMaxFrames || packed_bytes(count, maxFrames) > ((uint64_t)1 << 32))
        return -1;
    // (count == 0 admits no maxRecords >= maxFrames: its ticket is complete and nothing is written)
    if (count > 0 &&
        (!dense_ok(count, maxFrames, maxRecords) || streams_bytes(count, maxRecords) >= ((uint64_t)1 << 32)))
        return -1;
    return (long long)Engine::global()->stream_rows_async(deviceRows, stride, deviceStarts, deviceEnds, count,
                                                          maxFrames, count ? maxRecords : 0, pinnedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_frames_recv_streams(const SgpuDecoder* decoders, unsigned decoderCount,
                                                      const void* heads, unsigned maxFrames, unsigned maxRecords,
                                                      const void* deviceRows, size_t stride, unsigned count,
                                                      SiameseResult* results, unsigned* consumedOut,
                                                      unsigned* rowsOut, unsigned* acceptedOut)
{
    return recv_dense_rows(decoders, decoderCount, heads, maxFrames, maxRecords, deviceRows, stride, count, results,
                           true, consumedOut, rowsOut, acceptedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_pack_frames(SgpuEncoder encoder, unsigned flow, unsigned firstPacketNum,
                                                      unsigned originalCount, const SgpuRecoveryPacket* recovery,
                                                      unsigned recoveryCount, void* deviceDst, size_t stride,
                                                      unsigned maxRows, unsigned* deviceLens, SiameseResult* results,
                                                      unsigned* rowsOut, unsigned* framesOut)
{
    if (rowsOut)
        *rowsOut = 0;
    if (framesOut)
        *framesOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    if (!encoder || !rowsOut || !framesOut || !frame_rows_ok(maxRows, dst, stride, lens) || flow > kFrameMaxFlow ||
        firstPacketNum > SIAMESE_PACKET_NUM_MAX || (!recovery && recoveryCount))
        return Siamese_InvalidInput;
    EncoderCore& core = BE(encoder)->core;
    std::vector<EncoderCore::PackRecovery> rec(recoveryCount);
    for (unsigned k = 0; k < recoveryCount; ++k) {
        if (recovery[k].Producer != &core.program())
            return Siamese_InvalidInput;
        rec[k].data = (uint64_t)(uintptr_t)recovery[k].DeviceData;
        rec[k].bytes = recovery[k].DataBytes;
    }
    return core.pack_frames(flow, firstPacketNum, originalCount, rec.data(), recoveryCount, dst, (uint64_t)stride,
                            maxRows, lens, results, rowsOut, framesOut);
}

// ---- ARQ: acknowledgements and retransmissions (arq.cpp) ---------------------

SIAMESE_EXPORT SiameseResult sgpu_decoder_ack(SgpuDecoder decoder, void* buffer, unsigned byteLimit,
                                              unsigned* usedOut)
{
    if (!decoder || BD(decoder)->core.ge_pending() || !buffer || !usedOut || byteLimit < SIAMESE_ACK_MIN_BYTES)
        return Siamese_InvalidInput;
    return BD(decoder)->core.acknowledgement(static_cast<uint8_t*>(buffer), byteLimit, *usedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_acknowledge(SgpuEncoder encoder, const void* buffer, unsigned bytes,
                                                      unsigned* nextExpectedOut)
{
    if (!encoder || !buffer || bytes < 1 || !nextExpectedOut)
        return Siamese_InvalidInput;
    return BE(encoder)->core.acknowledge(static_cast<const uint8_t*>(buffer), bytes, *nextExpectedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_retransmit(SgpuEncoder encoder, SiameseOriginalPacket* out)
{
    if (!encoder || !out)
        return Siamese_InvalidInput;
    return BE(encoder)->core.retransmit(*out);
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_stats(SgpuEncoder encoder, uint64_t* statsOut, unsigned statsCount)
{
    if (!encoder || !statsOut || statsCount <= 0)
        return Siamese_InvalidInput;
    return BE(encoder)->core.stats(statsOut, statsCount);
}

SIAMESE_EXPORT SiameseResult sgpu_decoder_stats(SgpuDecoder decoder, uint64_t* statsOut, unsigned statsCount)
{
    if (!decoder || BD(decoder)->core.ge_pending() || !statsOut || statsCount <= 0)
        return Siamese_InvalidInput;
    return BD(decoder)->core.stats(statsOut, statsCount);
}

SIAMESE_EXPORT unsigned sgpu_frame_write_ack(unsigned flow, const void* msg, unsigned bytes, void* out,
                                             unsigned capacity)
{
    static_assert(SGPU_FRAME_ACK == kFrameAck, "SGPU_FRAME_ACK");
    return frame_write_ack(flow, static_cast<const uint8_t*>(msg), bytes, static_cast<uint8_t*>(out), capacity);
}

SIAMESE_EXPORT SiameseResult sgpu_decoders_ack_frames(const SgpuDecoder* decoders, unsigned count,
                                                      const unsigned* flows, unsigned byteLimit, void* deviceDst,
                                                      size_t stride, unsigned* deviceLens, SiameseResult* results,
                                                      unsigned* queuedOut)
{
    if (queuedOut)
        *queuedOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    // (a message has byteLimit bytes at most: a frame of that many must fit the row)
    if (((!decoders || !flows) && count) || !frame_rows_ok(count, dst, stride, lens) ||
        byteLimit < SIAMESE_ACK_MIN_BYTES || byteLimit > kFrameMaxLength - kFrameAckInner ||
        (uint64_t)frame_header_bytes(kFrameAck, byteLimit) + byteLimit > stride)
        return Siamese_InvalidInput;
    for (unsigned k = 0; k < count; ++k)
        if (!decoders[k] || BD(decoders[k])->core.ge_pending() || flows[k] > kFrameMaxFlow)
            return Siamese_InvalidInput;
    std::vector<uint8_t> msg(byteLimit);
    const uint8_t none[kFrameMaxHeader] = {};
    unsigned queued = 0;
    SiameseResult status = Siamese_Success;
    for (unsigned k = 0; k < count; ++k) {
        DecoderCore& core = BD(decoders[k])->core;
        unsigned used = 0;
        SiameseResult r = core.acknowledgement(msg.data(), byteLimit, used);
        if (r == Siamese_Success && (used < 1 || used > byteLimit))
            r = Siamese_Disabled;   // (no acknowledgement is empty or longer than its limit)
        const uint64_t row = dst + (uint64_t)k * stride, len = lens + (uint64_t)k * 4;
        if (r == Siamese_Success) {
            uint8_t hdr[kFrameMaxHeader] = {};
            const unsigned h = frame_write_ack_header(flows[k], used, hdr);
            core.program().frame_literal(msg.data(), used, hdr, h, row, len, (uint64_t)stride);
            ++queued;
        } else {
            // nothing to send (nothing received yet: NeedMoreData): a zero length, the row untouched
            core.program().frame(0, 0, none, 0, row, len, (uint64_t)stride);
            if (r != Siamese_NeedMoreData && status == Siamese_Success)
                status = r;
        }
        if (results)
            results[k] = r;
    }
    Engine::global()->count_ack_frames(queued);
    if (queuedOut)
        *queuedOut = queued;
    return status;
}

SIAMESE_EXPORT SiameseResult sgpu_encoder_retransmit_frames(SgpuEncoder encoder, unsigned flow, unsigned maxPackets,
                                                            void* deviceDst, size_t stride, unsigned maxRows,
                                                            unsigned* deviceLens, unsigned* packetNumsOut,
                                                            unsigned* rowsOut, unsigned* framesOut)
{
    if (rowsOut)
        *rowsOut = 0;
    if (framesOut)
        *framesOut = 0;
    const uint64_t dst = (uint64_t)(uintptr_t)deviceDst, lens = (uint64_t)(uintptr_t)deviceLens;
    if (!encoder || !rowsOut || !framesOut || !frame_rows_ok(maxRows, dst, stride, lens) || flow > kFrameMaxFlow)
        return Siamese_InvalidInput;
    return BE(encoder)->core.retransmit_frames(flow, maxPackets, dst, (uint64_t)stride, maxRows, lens, packetNumsOut,
                                               rowsOut, framesOut);
}

namespace {
static_assert(SGPU_ROW_TRUNCATED == kRowTruncated && SGPU_PACKED_ACKS_DROPPED == kPackedAcksDropped,
              "duplex scan values");

inline bool duplex_ok(unsigned maxFrames, unsigned ackSlots, unsigned ackBytes)
{
    return maxFrames >= 1 && maxFrames <= kPackedMaxFrames && ackSlots >= 1 && ackSlots <= maxFrames &&
           ackBytes >= kAckSlotBytesMin && ackBytes <= kAckSlotBytesMax && (ackBytes & 15u) == 0;
}

// One record of a duplex scan's row, copied from the caller's memory, for sgpu_frames_recv_duplex and
// sgpu_frames_recv_duplex_dense: an ack goes from its slot to encoders[Flow], anything else to
// decoders[Flow].  acks = the ack records met in this row before this one (counted here); rowSlots = the
// row's slot 0, of which rowSlotCount slots may be read; rowDev = the row's device address.
inline SiameseResult route_duplex_head(const SgpuDecoder* decoders, unsigned decoderCount,
                                       const SgpuEncoder* encoders, unsigned encoderCount, const PackedHead& h,
                                       uint64_t stride, unsigned ackSlots, unsigned ackBytes, unsigned& acks,
                                       const uint8_t* rowSlots, unsigned rowSlotCount, uint64_t rowDev,
                                       unsigned* nextOut, unsigned* accepted)
{
    SiameseResult r = Siamese_InvalidInput;
    if (h.type == kFrameAck) {
        // a truncated message is never handed on: cut short it states another loss list
        SgpuEncoder e = h.flow < encoderCount ? encoders[h.flow] : nullptr;
        if (ack_head_valid(h, stride, ackSlots, ackBytes, acks) && h.status == kRowOk && h.packetNum < rowSlotCount &&
            e) {
            uint8_t msg[kAckSlotBytesMax];
            std::memcpy(msg, rowSlots + (size_t)h.packetNum * ackBytes, h.dataBytes);
            unsigned next = 0;
            r = BE(e)->core.acknowledge(msg, h.dataBytes, next);
            if (nextOut)
                *nextOut = next;
            ++*accepted;
        }
        ++acks;
    } else if (packed_head_valid(h, stride))
        r = route_head(decoders, decoderCount, h, rowDev + h.offset + h.headerBytes, accepted);
    return r;
}

// the sizes sgpu_frames_scan_duplex_dense and sgpu_frames_recv_duplex_dense share
inline bool duplex_dense_ok(unsigned count, unsigned maxFrames, unsigned ackSlots, unsigned ackBytes,
                            unsigned maxRecords, unsigned maxAcks)
{
    return duplex_ok(maxFrames, ackSlots, ackBytes) && maxRecords >= maxFrames &&
           (uint64_t)maxRecords <= (uint64_t)count * maxFrames && maxAcks >= ackSlots &&
           (uint64_t)maxAcks <= (uint64_t)count * ackSlots &&
           duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes) < ((uint64_t)1 << 32);
}
} // namespace

SIAMESE_EXPORT size_t sgpu_frames_duplex_bytes(unsigned count, unsigned maxFrames, unsigned ackSlots,
                                               unsigned ackBytes)
{
    return duplex_ok(maxFrames, ackSlots, ackBytes) ? (size_t)duplex_bytes(count, maxFrames, ackSlots, ackBytes) : 0;
}

SIAMESE_EXPORT size_t sgpu_frames_duplex_slots(unsigned count, unsigned maxFrames)
{
    return maxFrames >= 1 && maxFrames <= kPackedMaxFrames ? (size_t)duplex_slots_offset(count, maxFrames) : 0;
}

SIAMESE_EXPORT long long sgpu_frames_scan_duplex(const void* deviceRows, size_t stride, const unsigned* deviceLens,
                                                 unsigned count, unsigned maxFrames, unsigned ackSlots,
                                                 unsigned ackBytes, void* pinnedOut)
{
    if (!g_batchReady || !rows_ok(deviceRows, stride, count) || ((uintptr_t)deviceLens & 3) ||
        ((uintptr_t)pinnedOut & 15) || (!pinnedOut && count > 0) || !duplex_ok(maxFrames, ackSlots, ackBytes) ||
        duplex_bytes(count, maxFrames, ackSlots, ackBytes) > ((uint64_t)1 << 32))
        return -1;
    return (long long)Engine::global()->duplex_rows_async(deviceRows, stride, deviceLens, count, maxFrames, ackSlots,
                                                          ackBytes, pinnedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_frames_recv_duplex(const SgpuDecoder* decoders, unsigned decoderCount,
                                                     const SgpuEncoder* encoders, unsigned encoderCount,
                                                     const void* heads, unsigned maxFrames, unsigned ackSlots,
                                                     unsigned ackBytes, const void* deviceRows, size_t stride,
                                                     unsigned count, SiameseResult* results,
                                                     unsigned* nextExpectedOut, unsigned* acceptedOut)
{
    if (!acceptedOut)
        return Siamese_InvalidInput;
    *acceptedOut = 0;
    if (!rows_ok(deviceRows, stride, count) || (!heads && count > 0) || (!decoders && decoderCount) ||
        (!encoders && encoderCount) || ((uintptr_t)heads & 3) || !duplex_ok(maxFrames, ackSlots, ackBytes))
        return Siamese_InvalidInput;
    const uint64_t dev = (uint64_t)(uintptr_t)deviceRows;
    const uint8_t* recs = static_cast<const uint8_t*>(heads);
    const uint8_t* words = recs + (size_t)count * maxFrames * sizeof(PackedHead);
    const uint8_t* slots = recs + (size_t)duplex_slots_offset(count, maxFrames);
    unsigned accepted = 0;
    SiameseResult status = Siamese_Success;
    for (unsigned k = 0; k < count; ++k) {
        // (the words, records and slots are the caller's memory: each is copied, checked and only then used)
        uint32_t word;
        std::memcpy(&word, words + (size_t)k * 4, 4);
        SiameseResult* res = results ? results + (size_t)k * maxFrames : nullptr;
        for (unsigned j = 0; res && j < maxFrames; ++j)
            res[j] = Siamese_NeedMoreData;
        unsigned n = word & kPackedCountMask;
        bool malformed = (word & kPackedMalformed) != 0;
        if (n > maxFrames) {   // (no scan writes such a word: none of the row's records is used)
            n = 0;
            malformed = true;
        }
        unsigned acks = 0;   // ack records met in this row
        for (unsigned j = 0; j < n; ++j) {
            PackedHead h;
            std::memcpy(&h, recs + ((size_t)k * maxFrames + j) * sizeof(h), sizeof(h));
            const SiameseResult r = route_duplex_head(
                decoders, decoderCount, encoders, encoderCount, h, stride, ackSlots, ackBytes, acks,
                slots + (size_t)k * ackSlots * ackBytes, ackSlots, dev + (uint64_t)k * stride,
                nextExpectedOut ? nextExpectedOut + (size_t)k * maxFrames + j : nullptr, &accepted);
            if (res)
                res[j] = r;
            if (r != Siamese_Success && r != Siamese_NeedMoreData && status == Siamese_Success)
                status = r;
        }
        if (malformed) {   // the frame the walk stopped at: the slot after the row's last record, if there is one
            if (res && n < maxFrames)
                res[n] = Siamese_InvalidInput;
            if (status == Siamese_Success)
                status = Siamese_InvalidInput;
        }
    }
    *acceptedOut = accepted;
    return status;
}

SIAMESE_EXPORT size_t sgpu_frames_duplex_dense_bytes(unsigned count, unsigned maxRecords, unsigned maxAcks,
                                                     unsigned ackBytes)
{
    // (what no maxFrames and ackSlots allow: fewer than one record or slot, more than 256 per row)
    if (maxRecords < 1 || (uint64_t)maxRecords > (uint64_t)count * kPackedMaxFrames || maxAcks < 1 ||
        (uint64_t)maxAcks > (uint64_t)count * kPackedMaxFrames || !duplex_ok(1, 1, ackBytes) ||
        duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes) >= ((uint64_t)1 << 32))
        return 0;
    return (size_t)duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes);
}

SIAMESE_EXPORT size_t sgpu_frames_duplex_dense_acks(unsigned count, unsigned maxRecords)
{
    return maxRecords >= 1 && (uint64_t)maxRecords <= (uint64_t)count * kPackedMaxFrames
               ? (size_t)duplex_dense_acks_offset(count, maxRecords)
               : 0;
}

SIAMESE_EXPORT size_t sgpu_frames_duplex_dense_slots(unsigned count, unsigned maxRecords)
{
    return maxRecords >= 1 && (uint64_t)maxRecords <= (uint64_t)count * kPackedMaxFrames
               ? (size_t)duplex_dense_slots_offset(count, maxRecords)
               : 0;
}

SIAMESE_EXPORT long long sgpu_frames_scan_duplex_dense(const void* deviceRows, size_t stride,
                                                       const unsigned* deviceLens, unsigned count,
                                                       unsigned maxFrames, unsigned ackSlots, unsigned ackBytes,
                                                       unsigned maxRecords, unsigned maxAcks, void* pinnedOut)
{
    if (!g_batchReady || !rows_ok(deviceRows, stride, count) || ((uintptr_t)deviceLens & 3) ||
        ((uintptr_t)pinnedOut & 15) || (!pinnedOut && count > 0) || !duplex_ok(maxFrames, ackSlots, ackBytes) ||
        duplex_bytes(count, maxFrames, ackSlots, ackBytes) > ((uint64_t)1 << 32))
        return -1;
    // (count == 0 admits no maxRecords >= maxFrames: its ticket is complete and nothing is written)
    if (count > 0 && !duplex_dense_ok(count, maxFrames, ackSlots, ackBytes, maxRecords, maxAcks))
        return -1;
    return (long long)Engine::global()->duplex_dense_rows_async(deviceRows, stride, deviceLens, count, maxFrames,
                                                                ackSlots, ackBytes, count ? maxRecords : 0,
                                                                count ? maxAcks : 0, pinnedOut);
}

namespace {
// sgpu_frames_recv_duplex_dense and, with the next words behind the dense part (streams) and consumedOut,
// sgpu_frames_recv_duplex_streams
SiameseResult recv_duplex_dense_rows(const SgpuDecoder* decoders, unsigned decoderCount, const SgpuEncoder* encoders,
                                     unsigned encoderCount, const void* heads, unsigned maxFrames, unsigned ackSlots,
                                     unsigned ackBytes, unsigned maxRecords, unsigned maxAcks, const void* deviceRows,
                                     size_t stride, unsigned count, SiameseResult* results, unsigned* nextExpectedOut,
                                     bool streams, unsigned* consumedOut, unsigned* rowsOut, unsigned* acceptedOut)
{
    if (rowsOut)
        *rowsOut = 0;
    if (!acceptedOut)
        return Siamese_InvalidInput;
    *acceptedOut = 0;
    if (!rowsOut || !rows_ok(deviceRows, stride, count) || (!heads && count > 0) || (!decoders && decoderCount) ||
        (!encoders && encoderCount) || ((uintptr_t)heads & 3) || !duplex_ok(maxFrames, ackSlots, ackBytes) ||
        (count > 0 && !duplex_dense_ok(count, maxFrames, ackSlots, ackBytes, maxRecords, maxAcks)) ||
        (streams && !consumedOut && count > 0))
        return Siamese_InvalidInput;
    if (count == 0)
        return Siamese_Success;
    for (unsigned i = 0; results && i < maxRecords; ++i)
        results[i] = Siamese_NeedMoreData;
    // (the output is the caller's memory: every word, record and slot is copied, checked and only then used)
    const uint64_t dev = (uint64_t)(uintptr_t)deviceRows;
    const uint8_t* base = static_cast<const uint8_t*>(heads);
    const uint8_t* words = base + 16;
    const uint8_t* starts = words + (size_t)count * 4;
    const uint8_t* recs = base + (size_t)dense_records_offset(count);
    const uint8_t* astarts = base + (size_t)duplex_dense_acks_offset(count, maxRecords);
    const uint8_t* slots = base + (size_t)duplex_dense_slots_offset(count, maxRecords);
    const uint8_t* nextWords =
        streams ? base + (size_t)duplex_streams_next_offset(count, maxRecords, maxAcks, ackBytes) : nullptr;
    uint32_t info[4];
    std::memcpy(info, base, sizeof(info));
    const uint32_t W = info[1], c = info[2], WA = info[3];
    if (c > count || W > maxRecords || WA > maxAcks)
        return Siamese_InvalidInput;
    unsigned accepted = 0;
    SiameseResult status = Siamese_Success;
    uint32_t at = 0, aat = 0;   // start[k] and astart[k], checked
    std::memcpy(&at, starts, 4);
    std::memcpy(&aat, astarts, 4);
    bool forged = at != 0 || aat != 0;
    unsigned k = 0;
    for (; !forged && k < c; ++k) {
        uint32_t word, next, anext;
        std::memcpy(&word, words + (size_t)k * 4, 4);
        std::memcpy(&next, starts + (size_t)(k + 1) * 4, 4);
        std::memcpy(&anext, astarts + (size_t)(k + 1) * 4, 4);
        unsigned n = word & kPackedCountMask;
        bool malformed = (word & kPackedMalformed) != 0;
        const unsigned span = n < maxFrames ? n : maxFrames;
        // the row's records are [at, next): non-decreasing, as many as its word says, and before W
        if (next < at || next - at != span || next > W) {
            forged = true;
            break;
        }
        // the row's slots are [aat, anext): non-decreasing, one for each of its ack records that names a
        // slot, and before WA
        unsigned named = 0;
        for (unsigned j = 0; j < span; ++j) {
            PackedHead h;
            std::memcpy(&h, recs + ((size_t)at + j) * sizeof(h), sizeof(h));
            named += h.type == kFrameAck && h.packetNum < ackSlots;
        }
        if (anext < aat || anext - aat != named || anext > WA) {
            forged = true;
            break;
        }
        if (n > maxFrames) {   // (no scan writes such a word: none of the row's records is used)
            n = 0;
            malformed = true;
        }
        uint32_t resume = 0;
        if (nextWords) {
            // where the row's next scan starts: within the row, and not before the end of its last record
            std::memcpy(&resume, nextWords + (size_t)k * 4, 4);
            uint64_t least = 0;
            if (n > 0) {
                PackedHead h;
                std::memcpy(&h, recs + ((size_t)at + n - 1) * sizeof(h), sizeof(h));
                least = (uint64_t)h.offset + h.headerBytes + h.dataBytes;
            }
            if (resume > stride || resume < least) {
                forged = true;
                break;
            }
        }
        unsigned acks = 0;   // ack records met in this row
        for (unsigned j = 0; j < n; ++j) {
            PackedHead h;
            std::memcpy(&h, recs + ((size_t)at + j) * sizeof(h), sizeof(h));
            const SiameseResult r = route_duplex_head(
                decoders, decoderCount, encoders, encoderCount, h, stride, ackSlots, ackBytes, acks,
                slots + (size_t)aat * ackBytes, named, dev + (uint64_t)k * stride,
                nextExpectedOut ? nextExpectedOut + at + j : nullptr, &accepted);
            if (results)
                results[at + j] = r;
            if (r != Siamese_Success && r != Siamese_NeedMoreData && status == Siamese_Success)
                status = r;
        }
        if (malformed && status == Siamese_Success)   // (the frame the walk stopped at has no slot here)
            status = Siamese_InvalidInput;
        if (nextWords)
            consumedOut[k] = resume;
        at = next;
        aat = anext;
    }
    if (!forged && (at != W || aat != WA))
        forged = true;
    *rowsOut = k;   // c, unless a table stopped the routing before it
    *acceptedOut = accepted;
    return forged ? Siamese_InvalidInput : status;
}
} // namespace

SIAMESE_EXPORT SiameseResult sgpu_frames_recv_duplex_dense(const SgpuDecoder* decoders, unsigned decoderCount,
                                                           const SgpuEncoder* encoders, unsigned encoderCount,
                                                           const void* heads, unsigned maxFrames, unsigned ackSlots,
                                                           unsigned ackBytes, unsigned maxRecords, unsigned maxAcks,
                                                           const void* deviceRows, size_t stride, unsigned count,
                                                           SiameseResult* results, unsigned* nextExpectedOut,
                                                           unsigned* rowsOut, unsigned* acceptedOut)
{
    return recv_duplex_dense_rows(decoders, decoderCount, encoders, encoderCount, heads, maxFrames, ackSlots,
                                  ackBytes, maxRecords, maxAcks, deviceRows, stride, count, results, nextExpectedOut,
                                  false, nullptr, rowsOut, acceptedOut);
}

static_assert(SGPU_STREAM_PARTIAL_DUPLEX == kStreamPartialDuplex &&
                  !(SGPU_STREAM_PARTIAL_DUPLEX &
                    (kPackedCountMask | kPackedMore | kPackedMalformed | kPackedAcksDropped)),
              "the duplex stream scan's row word");

SIAMESE_EXPORT size_t sgpu_frames_duplex_streams_bytes(unsigned count, unsigned maxRecords, unsigned maxAcks,
                                                       unsigned ackBytes)
{
    return sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes)
               ? (size_t)duplex_streams_bytes(count, maxRecords, maxAcks, ackBytes)
               : 0;
}

SIAMESE_EXPORT size_t sgpu_frames_duplex_streams_next(unsigned count, unsigned maxRecords, unsigned maxAcks,
                                                      unsigned ackBytes)
{
    return sgpu_frames_duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes)
               ? (size_t)duplex_streams_next_offset(count, maxRecords, maxAcks, ackBytes)
               : 0;
}

SIAMESE_EXPORT long long sgpu_frames_scan_duplex_streams(const void* deviceRows, size_t stride,
                                                         const unsigned* deviceStarts, const unsigned* deviceEnds,
                                                         unsigned count, unsigned maxFrames, unsigned ackSlots,
                                                         unsigned ackBytes, unsigned maxRecords, unsigned maxAcks,
                                                         void* pinnedOut)
{
    if (!g_batchReady || !rows_ok(deviceRows, stride, count) || ((uintptr_t)deviceStarts & 3) ||
        ((uintptr_t)deviceEnds & 3) || ((uintptr_t)pinnedOut & 15) || (!pinnedOut && count > 0) ||
        !duplex_ok(maxFrames, ackSlots, ackBytes) ||
        duplex_bytes(count, maxFrames, ackSlots, ackBytes) > ((uint64_t)1 << 32))
        return -1;
    // (count == 0 admits no maxRecords >= maxFrames: its ticket is complete and nothing is written)
    if (count > 0 && (!duplex_dense_ok(count, maxFrames, ackSlots, ackBytes, maxRecords, maxAcks) ||
                      duplex_streams_bytes(count, maxRecords, maxAcks, ackBytes) >= ((uint64_t)1 << 32)))
        return -1;
    return (long long)Engine::global()->duplex_stream_rows_async(deviceRows, stride, deviceStarts, deviceEnds, count,
                                                                 maxFrames, ackSlots, ackBytes,
                                                                 count ? maxRecords : 0, count ? maxAcks : 0,
                                                                 pinnedOut);
}

SIAMESE_EXPORT SiameseResult sgpu_frames_recv_duplex_streams(const SgpuDecoder* decoders, unsigned decoderCount,
                                                             const SgpuEncoder* encoders, unsigned encoderCount,
                                                             const void* heads, unsigned maxFrames,
                                                             unsigned ackSlots, unsigned ackBytes,
                                                             unsigned maxRecords, unsigned maxAcks,
                                                             const void* deviceRows, size_t stride, unsigned count,
                                                             SiameseResult* results, unsigned* nextExpectedOut,
                                                             unsigned* consumedOut, unsigned* rowsOut,
                                                             unsigned* acceptedOut)
{
    return recv_duplex_dense_rows(decoders, decoderCount, encoders, encoderCount, heads, maxFrames, ackSlots,
                                  ackBytes, maxRecords, maxAcks, deviceRows, stride, count, results, nextExpectedOut,
                                  true, consumedOut, rowsOut, acceptedOut);
}

SIAMESE_EXPORT long long sgpu_frames_send(unsigned count, const SgpuRecoveryPacket* packets, const unsigned* flows,
                                          void* pinnedOut, size_t capacity, size_t* bytesOut)
{
    if (!g_batchReady || !packets || !flows || !pinnedOut || !bytesOut)
        return -1;
    std::vector<const void*> srcs(count);
    std::vector<unsigned> lens(count), hlen(count);
    std::vector<uint8_t> hdr((size_t)count * 8);
    size_t total = 0;
    for (unsigned i = 0; i < count; ++i) {
        // (as sgpu_frame_write_header: an empty or oversized packet is no frame)
        if (!packets[i].DeviceData || flows[i] > kFrameMaxFlow || packets[i].DataBytes == 0 ||
            packets[i].DataBytes > SIAMESE_MAX_PACKET_BYTES)
            return -1;
        srcs[i] = packets[i].DeviceData;
        lens[i] = packets[i].DataBytes;
        hlen[i] = frame_write_header(kFrameRecovery, flows[i], 0, lens[i], hdr.data() + 8 * (size_t)i);
        if (hlen[i] > 8)
            return -1;
        total = (total + hlen[i] + lens[i] + 15) & ~(size_t)15;
    }
    *bytesOut = total;
    if (total > capacity)
        return -1;
    return (long long)Engine::global()->gather_async_framed(count, srcs.data(), lens.data(), hdr.data(), hlen.data(),
                                                            pinnedOut);
}

SIAMESE_EXPORT void sgpu_timing(int enable, int reset, double* execMs, double* totalMs)
{
    be_timing_enable(enable != 0);
    if (execMs)
        *execMs = be_timing_kernel_ms(kBeExec);
    if (totalMs)
        *totalMs = be_timing_total_ms();
    if (reset)
        be_timing_reset();
}

SIAMESE_EXPORT void sgpu_timing_kernels(double* msOut, unsigned count)
{
    for (unsigned k = 0; k < count && k < kBeKernelKinds; ++k)
        msOut[k] = be_timing_kernel_ms((BeKernel)k);
}

SIAMESE_EXPORT void sgpu_engine_stats_ex(uint64_t* out, unsigned count)
{
    const EngineStats s = Engine::global()->stats();
    const Engine* e = Engine::global();
    const uint64_t v[44] = {s.flushes,    s.launches,    s.ops,        s.terms,    s.solves,
                            s.ingests,    s.uploadBytes, s.refOpBytes, s.outBytes, s.solveBytes,
                            s.assembleNs, s.waitNs,      s.completeNs, s.reclaimNs,
                            s.execLaunches, s.ldpcBytes, s.execUniqueBytes,
                            s.geJobs,     s.geChained,   s.geRetried,  s.geChainedWide,
                            s.delivers,   s.frames,      s.scans,      Engine::global()->walks(),
                            s.relays,     Engine::global()->packs(),
                            Engine::global()->duplexes(), Engine::global()->ack_frames(),
                            Engine::global()->concats(),
                            e->rows_shape(0), e->rows_shape(1), e->rows_shape(2), e->rows_shape(3),
                            e->rows_shape(4), be_exec_stage_cap(),
                            e->denses(),  s.gePivoted,   s.geSingular,
                            e->duplex_denses(), e->solves_flagged(), e->solves_cut(), e->streams(),
                            e->duplex_streams()};
    for (unsigned k = 0; k < count && k < 44; ++k)
        out[k] = v[k];
}

SIAMESE_EXPORT void sgpu_measure_unique(int on)
{
    Engine::set_measure_unique(on != 0);
}

SIAMESE_EXPORT void sgpu_engine_stats(uint64_t* out15)
{
    const EngineStats s = Engine::global()->stats();
    const uint64_t v[15] = {s.flushes,    s.launches,    s.ops,        s.terms,    s.solves,
                            s.ingests,    s.uploadBytes, s.refOpBytes, s.outBytes, s.solveBytes,
                            s.assembleNs, s.waitNs,      s.completeNs, s.reclaimNs,
                            s.execLaunches};
    std::memcpy(out15, v, sizeof(v));
}

SIAMESE_EXPORT uint64_t sgpu_arena_bytes(void)
{
    return Engine::global()->arena_bytes();
}

SIAMESE_EXPORT int sgpu_arena_reserve(size_t bytes)
{
    if (!g_batchReady)
        return -1;
    return Engine::global()->reserve(bytes) ? 0 : -1;
}

} // extern "C"
