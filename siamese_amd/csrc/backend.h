// backend.h -- the only interface between the host control plane and the
// device.  libsiamese_amd.so implements it with HIP on gfx950
// (backend_hip.hip).  A host simulation of the same contract exists ONLY for
// the CPU test suite (tools/backend_hostsim.cpp, linked into
// tests/hostsim/libsiamese_hostsim.so), never in the shipped library.
#pragma once

#include "ops.h"
#include <cstddef>
#include <cstdint>

namespace sgpu {

/// Initialise the device (HIP device index; <0 = current).  Returns false
/// with a message in *err when no usable MI355X device exists.
bool be_init(int device, const char** err);
const char* be_name();

void* be_dev_alloc(size_t bytes);
void be_dev_free(void* p);
void* be_host_alloc(size_t bytes);   // page-locked
/// Page-locked, mapped and coherent host memory: kernels read and write it
/// directly (zero-copy uploads, k_hostcopy downloads), and a buffer rewritten
/// between submissions is never seen stale through a device cache.
void* be_host_alloc_mapped(size_t bytes);
/// The device's address of page-locked host memory (kernels read it over
/// the bus: zero-copy).
void* be_host_device_ptr(void* host);
void be_host_free(void* p);

// All transfers and launches are asynchronous on the engine's stream.
void be_h2d(void* dst, const void* src, size_t bytes);
void be_d2h(void* dst, const void* src, size_t bytes);
void be_memset(void* dst, int value, size_t bytes);
/// Copies between device memory and page-locked host memory (be_host_alloc):
/// small totals run as one kernel on the engine's stream (no copy-engine
/// hand-off, whose cross-queue wait costs more than the bytes on the
/// latency-bound single-stream path), large ones as DMA.
struct BeCopy
{
    uint64_t dst, src;
    uint64_t bytes;
};
constexpr unsigned kBeCopyMax = 8;   // ranges per be_copy_pinned call
void be_copy_pinned(const BeCopy* ranges, unsigned count, bool toDevice);
/// The same ranges with a device-readable copy of the list (devList: each
/// range's host side as the device addresses it, be_host_device_ptr), so
/// that any number of small ranges takes one kernel launch; null devList, or
/// ranges too large for a kernel, fall back to be_copy_pinned.
void be_copy_list(const BeCopy* ranges, const void* devList, unsigned count, bool toDevice);

/// One k_ingest launch.  One wave per (descriptor, kIngestChunkBytes chunk):
/// maxBytes is the largest hdrLen + bytes among the descriptors (sizes the
/// grid).  blocks: the k_ingest block table (nblocks entries, descriptor << 4
/// | 4-symbol group of its run), or null for runs of one (one per wave).
struct BeIngest
{
    const IngestDesc* descs;
    uint32_t count;
    uint32_t maxBytes;
    const uint32_t* blocks = nullptr;
    uint32_t nblocks = 0;
};
void be_launch_ingest(const BeIngest& ingest);
/// `stream`: the instruction words of every segment (see ExecItem).
/// `acct`: device counter the executor adds the reference's source bytes of
/// the terms it expands itself (sum updates, LDPC picks) to (ops.h).
/// `maxWindow`: the largest OP_ROWS window (entries) among the launched
/// segments, kNoRows when none has a row batch (sizes the LDS stage).
/// `results`: the submission's result words, which gate the rows of an
/// OP_ROWS batch whose GfOp.termBegin is non-zero (1 + the word; a zero word
/// skips the rows: a chained device elimination that failed, ops.h GeDesc).
void be_launch_exec(const void* stream, const ExecItem* items, uint32_t count, uint64_t* acct,
                    const uint32_t* results, uint32_t maxWindow);
/// Window elements the executor's LDS stage holds at most (fixed by be_init
/// from the device's LDS and the kernel's static share of it): an OP_ROWS
/// batch that reads more elements (GfOp.valid - stageLo) reads those past the
/// stage from memory.  0: the backend has no stage, no batch exceeds it.
uint32_t be_exec_stage_cap();
/// Wide rows' LDPC picks (ops.h LdpcItem), one workgroup per item; adds the
/// reference's source bytes of the picks (min(len, n) each) to acct[0].
/// gates (or null: every item runs): one word per item, 0 or 1 + a word of
/// `results`; an item whose word reads zero does nothing (a chained decode's
/// wide rows, ops.h LdpcItem).  The caller orders a gated launch after the job
/// that writes those words (be_join_ge).
void be_launch_ldpc(const LdpcItem* items, uint32_t count, uint64_t* acct, const uint32_t* gates = nullptr,
                    const uint32_t* results = nullptr);
/// The triangular solves (reference SiameseDecoder.cpp:1065-1238), one
/// workgroup per SolveItem: every tile first solves bytes 0..3 of its rows
/// to learn the recovered lengths, the tile-0 item writes them to `results`
/// and adds acct[0] += the reference's source bytes of each
/// back-substitution step the solve completes (:1131-1212), acct[1] += the
/// recovered bytes it outputs.  maxRows: largest m among the solves (sizes
/// the LDS staging).
void be_launch_solve(const SolveDesc* solves, const SolveRow* rows, const uint8_t* coef, uint32_t* results,
                     const SolveItem* items, uint32_t count, uint32_t maxRows, uint64_t* acct,
                     uint32_t solveBegin, uint32_t solveCount);

/// Device recovery-matrix generation + elimination (ops.h GeDesc): one job
/// per desc, its input at in + desc.in, its output in results + desc.result;
/// a kGeChained job that succeeds also writes its solve's coefficients
/// (coef + solveCoef) and its SolveRows (rows + solveRow) in pivot order,
/// read from rowsIn + solveRow.  Reads nothing any other launch of the flush
/// writes.  maxRows / maxCols: the largest job of the launch (sizes its LDS).
struct BeGe
{
    const GeDesc* descs;
    const uint8_t* in;
    uint32_t count;
    uint32_t* results;
    const SolveRow* rowsIn;   // `rows` itself, or the same rows in the mapped upload
    SolveRow* rows;
    uint8_t* coef;
    uint32_t maxRows, maxCols;
};
/// Where the jobs of a submission run.  Both placements fork the side stream
/// from the codec stream first; be_join_ge() puts the codec stream behind the
/// side stream again, after which every launch (and the results' download)
/// sees the jobs' outputs.
enum class GePlace
{
    /// In line on the codec stream, after `head` when it has bytes (`head`
    /// belongs to this placement alone; kSideStream ignores it): a pinned
    /// H2D copy that brings the jobs' descriptors, inputs, rows and
    /// coefficients into place.  No bytes: descs, in and rowsIn are mapped
    /// pinned memory (be_host_device_ptr) and the jobs need no copy at all.
    /// The caller puts the rest of the upload and k_ingest beside the jobs
    /// with be_side_upload_ingest.
    kCodecStream,
    /// On the side stream, beside whatever the codec stream queues until
    /// be_join_ge() (a submission whose upload is not copied: nothing to put
    /// beside the jobs but the codec stream's own next launches).
    kSideStream,
};
void be_launch_ge(const BeGe& ge, GePlace place, const BeCopy& head = BeCopy{0, 0, 0});
/// After be_launch_ge(GePlace::kCodecStream): the rest of the upload (when
/// it has bytes) and k_ingest on the side stream, beside the jobs.
void be_side_upload_ingest(const BeCopy& rest, const BeIngest& ingest);
void be_join_ge();

/// Packets into caller-owned rows (ops.h DeliverItem), one wave per (item,
/// kIngestChunkBytes chunk of its row): each row gets its packet's payload
/// and a zero tail, and its length word (zero for an absent packet or one
/// whose prefix does not fit).  maxStride: the largest row among the items
/// in bytes, saturated to 32 bits (sizes the grid).  The caller queues it
/// after every launch that writes the symbols (and after be_join_ge()).
void be_launch_deliver(const DeliverItem* items, uint32_t count, uint32_t maxStride);
/// A sender's packets framed into caller-owned rows (ops.h FrameItem), the
/// grid and maxStride as be_launch_deliver's: each row gets its literal
/// header, the packet and a zero tail, and its length word when the item has
/// one (lenBase, and an untouched row, for an absent packet).  Queued beside
/// be_launch_deliver.
void be_launch_frame(const FrameItem* items, uint32_t count, uint32_t maxStride);
/// A decoder's packets forwarded as originals' wire frames into caller-owned
/// rows (ops.h RelayItem), the grid and maxStride as be_launch_deliver's: each
/// row gets the frame header computed from the length read on the device, the
/// payload and a zero tail, and its length word (zero, and an untouched row,
/// for an absent packet; zero and a zeroed row for one that does not fit).
/// Queued beside be_launch_deliver.
void be_launch_relay(const RelayItem* items, uint32_t count, uint32_t maxStride);
/// A decoder's packets forwarded as wire frames, several to a row (ops.h
/// PackJob, PackItem, PlanRec): k_plan lays out every job's frames from the
/// lengths it reads on the device, into plan[0, count), and writes the jobs'
/// length words and info records; k_pack then writes every planned frame and
/// the zeros of its span.  plan is device memory of the submission, count
/// records, which the host never reads; maxStride is the longest row in bytes,
/// saturated at 2^32 - 1 (k_pack's grid).  Queued beside be_launch_deliver.
void be_launch_pack(const PackJob* jobs, uint32_t jobCount, const PackItem* items, uint32_t count, PlanRec* plan,
                    uint32_t maxStride);
/// A decoder's packets as one contiguous byte stream (ops.h ConcatJob,
/// ConcatItem, ConcatRec): k_offsets sums every job's lengths, read on the
/// device, into recs[0, count) and writes the jobs' offset words and info
/// records; k_concat then copies every delivered payload to its byte offset.
/// recs is device memory of the submission, count records, which the host
/// never reads; maxBytes is the longest symbol in bytes (k_concat's grid).
/// Queued beside be_launch_deliver.
void be_launch_concat(const ConcatJob* jobs, uint32_t jobCount, const ConcatItem* items, uint32_t count,
                      ConcatRec* recs, uint32_t maxBytes);

/// Block until all queued work has finished.  Returns false on a device fault.
bool be_sync();

/// A marker after all work queued so far.  be_fence_wait blocks (sleeping,
/// not spinning) until the device has passed it, returns false on a device
/// fault, and releases it.  The launcher thread creates fences, the
/// completer thread waits for them.
void* be_fence();
/// spinUs: poll this long before sleeping (latency-bound small flushes);
/// sleepPoll: poll with short sleeps instead of the runtime's blocking wait,
/// which spins on the core first (large flushes on a CPU-quota-bound host).
bool be_fence_wait(void* fence, unsigned spinUs, bool sleepPoll);

/// Transfer streams beside the codec stream (end-to-end packet flows).
/// be_stage_h2d copies host -> device on the staging stream right away (the
/// caller guarantees that no unfinished submission touches dst) and returns
/// a mark; be_wait_mark makes the codec stream wait for it on the device
/// (the host never blocks); be_mark_release recycles it once that wait has
/// been queued.  Null mark: the copy could not be queued.
void* be_stage_h2d(void* dst, const void* src, size_t bytes);
void be_wait_mark(void* mark);
void be_mark_release(void* mark);
/// Gather on the gather stream: upload `count` ingest descriptors (from
/// pinned descsHost to descsDev), pack their sources into devStage and copy
/// `bytes` of it to hostOut, without waiting (not even for the gather
/// stream).  Returns two marks: *packed is passed once the sources have been
/// read (be_wait_mark / be_mark_release, like a staging mark), *landed once
/// hostOut holds the bytes (be_mark_sync).  False if it could not be queued.
bool be_gather(const IngestDesc* descsHost, void* descsDev, uint32_t count, const void* devStage,
               void* hostOut, size_t bytes, void** packed, void** landed);
/// One k_scan launch on the gather stream (ops.h RowHead): one record per
/// row of rows + k * stride, k < count, into devStage (count * 32 bytes,
/// device memory), then one copy of the records to hostOut (pinned), without
/// waiting.  lens: the rows' length words in device memory, or null.  The
/// marks are be_gather's: *packed once the rows have been read, *landed once
/// hostOut holds the records.  False if it could not be queued.
bool be_scan_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, void* devStage,
                  void* hostOut, void** packed, void** landed);
/// One k_walk launch on the gather stream (ops.h PackedHead): maxFrames
/// records per row and then one word per row into devStage (packed_bytes(count,
/// maxFrames), device memory), then one copy of all of it to hostOut (pinned),
/// without waiting.  rows, stride, lens and the marks are be_scan_rows'.
bool be_walk_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, uint32_t maxFrames,
                  void* devStage, void* hostOut, void** packed, void** landed);
/// One k_ackwalk launch on the gather stream (ops.h kRowTruncated): k_walk's
/// records and row words, and ackSlots message slots of ackBytes bytes per row
/// from duplex_slots_offset(count, maxFrames) on, into devStage
/// (duplex_bytes(count, maxFrames, ackSlots, ackBytes), device memory, 16-byte
/// aligned), then one copy of all of it to hostOut (pinned), without waiting.
/// rows, stride, lens and the marks are be_scan_rows'.
bool be_ackwalk_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, uint32_t maxFrames,
                     uint32_t ackSlots, uint32_t ackBytes, void* devStage, void* hostOut, void** packed,
                     void** landed);
/// The packed scan in dense form (ops.h dense_bytes): three launches on the
/// gather stream -- k_walk's walk with the row's records into the scratch area
/// at dense_scratch_offset(count, maxRecords) and the row words into the output,
/// k_rowsum for the starts and the info words, k_compact for the records -- all
/// into devStage (dense_stage_bytes(count, maxFrames, maxRecords), device
/// memory, 16-byte aligned), then one copy of the first dense_bytes(count,
/// maxRecords) bytes to hostOut (pinned), without waiting.  rows, stride, lens
/// and the marks are be_scan_rows'.
bool be_dense_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, uint32_t maxFrames,
                   uint32_t maxRecords, void* devStage, void* hostOut, void** packed, void** landed);
/// The duplex scan in dense form (ops.h duplex_dense_bytes): four launches on
/// the gather stream -- k_ackwalk's walk with the row's records, slots and ack
/// count into the scratch areas (duplex_dense_scratch_*) and the row words into
/// the output, k_rowsum2 for both start tables and the info words, k_compact for
/// the records, k_slots for the slots -- all into devStage
/// (duplex_dense_stage_bytes(...), device memory, 16-byte aligned), then one copy
/// of the first duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes) bytes to
/// hostOut (pinned), without waiting.  rows, stride, lens and the marks are
/// be_scan_rows'.
bool be_duplex_dense_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count,
                          uint32_t maxFrames, uint32_t ackSlots, uint32_t ackBytes, uint32_t maxRecords,
                          uint32_t maxAcks, void* devStage, void* hostOut, void** packed, void** landed);
/// The scan of byte-stream rows (ops.h streams_bytes): three launches on the
/// gather stream -- k_streamwalk's walk of row bytes [starts[k], ends[k]) with
/// the row's records into the scratch area at streams_scratch_offset(count,
/// maxRecords), the row words into the output and the next words behind its
/// dense part, then k_rowsum and k_compact as in be_dense_rows -- all into
/// devStage (streams_stage_bytes(count, maxFrames, maxRecords), device memory,
/// 16-byte aligned), then one copy of the first streams_bytes(count, maxRecords)
/// bytes to hostOut (pinned), without waiting.  starts and ends: the rows' two
/// words in device memory, each or both null (0 and stride).  rows, stride and
/// the marks are be_scan_rows'.
bool be_stream_rows(const void* rows, uint64_t stride, const uint32_t* starts, const uint32_t* ends, uint32_t count,
                    uint32_t maxFrames, uint32_t maxRecords, void* devStage, void* hostOut, void** packed,
                    void** landed);
/// The scan of duplex byte-stream rows (ops.h duplex_streams_bytes): four
/// launches on the gather stream -- k_ackstreamwalk's walk of row bytes
/// [starts[k], ends[k]) with the row's records, slots and ack count into the
/// scratch areas (duplex_streams_scratch_*), the row words into the output and
/// the next words behind its dense part, then k_rowsum2, k_compact and k_slots
/// as in be_duplex_dense_rows -- all into devStage
/// (duplex_streams_stage_bytes(...), device memory, 16-byte aligned), then one
/// copy of the first duplex_streams_bytes(count, maxRecords, maxAcks, ackBytes)
/// bytes to hostOut (pinned), without waiting.  starts and ends are
/// be_stream_rows'; rows, stride and the marks are be_scan_rows'.
bool be_duplex_stream_rows(const void* rows, uint64_t stride, const uint32_t* starts, const uint32_t* ends,
                           uint32_t count, uint32_t maxFrames, uint32_t ackSlots, uint32_t ackBytes,
                           uint32_t maxRecords, uint32_t maxAcks, void* devStage, void* hostOut, void** packed,
                           void** landed);
/// Block until the device has passed `mark`, then recycle it; false on a
/// device fault.
bool be_mark_sync(void* mark);

/// Device-time accounting: every executor/solve launch is bracketed with
/// events; these return the accumulated milliseconds since the last reset.
/// Kernel classes of the per-launch device timing.
/// (kBeScan, kBeWalk, kBeAckWalk, kBeRowsum, kBeCompact, kBeRowsum2, kBeSlots, kBeStreamWalk and kBeAckStreamWalk
/// are bracketed on
/// the gather stream: be_sync waits for a bracket of those classes still in flight before it folds
/// it in; the dense scan's walk is counted as kBeWalk, the duplex dense scan's as kBeAckWalk and
/// its k_compact as kBeCompact; the stream scan's walk has its own class, its k_rowsum and k_compact are
/// counted as kBeRowsum and kBeCompact; the duplex stream scan's walk has its own class too, its k_rowsum2,
/// k_compact and k_slots are counted as kBeRowsum2, kBeCompact and kBeSlots)
enum BeKernel
{
    kBeIngest,
    kBeExec,
    kBeLdpc,
    kBeSolve,
    kBeGe,
    kBeDeliver,
    kBeFrame,
    kBeScan,
    kBeWalk,
    kBeRelay,
    kBePlan,
    kBePack,
    kBeAckWalk,
    kBeOffsets,
    kBeConcat,
    kBeRowsum,
    kBeCompact,
    kBeRowsum2,
    kBeSlots,
    kBeStreamWalk,
    kBeAckStreamWalk,
    kBeKernelKinds
};
void be_timing_enable(bool on);
/// Device milliseconds of one kernel class since the last reset.
double be_timing_kernel_ms(BeKernel kind);
void be_timing_reset();
double be_timing_total_ms();

} // namespace sgpu
