// ops.h -- descriptors handed from the host control plane to the MI355X
// kernels.  Plain POD, shared verbatim by host C++ and HIP device code.
//
// Execution model (see DESIGN.md "Device program"):
//   * Every codec instance (one encoder or one decoder) owns an ordered list
//     of ops.  Ops of different instances are independent.
//   * All symbol arithmetic is byte-column local (byte i of every operand
//     only meets byte i of the others), so the executor runs each instance's
//     op list once per 1 KiB byte tile, in parallel over (instance, tile),
//     with no synchronisation between workgroups.
//   * The triangular solve of a decode needs the recovered length prefix
//     (bytes 0..3) before it can truncate later rows, so it is a separate
//     pair of launches (solve_prefix, solve_main) between executor segments.
#pragma once

#include <cstdint>

namespace sgpu {

/// One source of a linear combination: contributes coeff * src[0, len).
struct GfTerm
{
    uint64_t src;     // device address
    uint32_t len;     // bytes read from src (host guarantees len <= op.n)
    uint8_t coeff;    // GF(256) multiplier; 1 = plain XOR
    uint8_t acc;      // accumulator 0 (direct) or 1 (multiplied by op.mix)
    uint16_t pad;
};

enum GfOpKind : uint32_t
{
    OP_LINCOMB = 1,   // dst[0,n) = keep(dst,valid) ^ acc0 ^ mix*acc1
    OP_LITERAL = 2,   // dst[n, n+valid) = literal bytes (<= 8)
    OP_ROWS = 3,      // a batch of Siamese rows of one codec (sum updates, rows)
    OP_COPIES = 4,    // independent copies dst[0,len) = src[0,len)
    OP_LINCOMBS = 5,  // independent OP_LINCOMBs (+ footer literals), one per wave
};

/// One op.  For OP_LINCOMB:
///   for i < n:  dst[i] = (i < valid ? dst[i] : 0) ^ sum_{acc0 terms} c*src[i]
///                        ^ mix * sum_{acc1 terms} c*src[i]
///   bytes of dst in [n, align16(n)) become zero and bytes at and beyond
///   align16(n) are left untouched.  Every symbol buffer therefore reads as
///   zero between its length and the end of its last 16-byte lane (k_ingest
///   and the solve keep the same rule), which the executor relies on when it
///   reads a term of length len < n.
/// For OP_LITERAL: writes `valid` (<= 8) bytes taken from `lit` at dst + n.
struct GfOp
{
    uint64_t dst;
    uint32_t n;
    uint32_t valid;
    uint32_t kind;
    uint32_t mix;
    union {
        struct {
            uint32_t termBegin;
            uint32_t termCount;
        };
        uint8_t lit[8];
    };
};
static_assert(sizeof(GfOp) == 32, "GfOp layout");
static_assert(sizeof(GfTerm) == 16, "GfTerm layout");

/// On the device a segment is one instruction stream of 16-byte words: each
/// op is its GfOp (2 words) followed, for OP_LINCOMB, by its termCount
/// GfTerm words.  On the device termBegin is the op's gate (every kind but
/// OP_LITERAL): 0, or 1 + a result word; the op is skipped when that word is
/// zero (a chained device elimination that failed, GeDesc kGeChained).  A workgroup streams through it
/// front to back, so one coalesced prefetch brings an op and its term list.
constexpr unsigned kOpWords = sizeof(GfOp) / 16;

/// OP_ROWS: a batch of Siamese rows of one codec (reference
/// SiameseEncoder.cpp:1046-1144 and :359-418, the decoder's elimination
/// SiameseDecoder.cpp:937-1063 and :1680-1739).  Everything symbol-sized is
/// expanded on the device: the lane-sum updates generate their own terms and
/// coefficients CX(column) / CX(column)^2 from a snapshot of the codec's
/// window, and each row generates its LDPC pair picks from PCG(row, n).  The
/// host sends O(1) words per row instead of a term per source.
///
/// Stream layout after the GfOp header (kind = OP_ROWS, n = rows R,
/// valid = window entries E, mix = sum updates U, termCount = block words,
/// dst low word = stageLo: the first window element the batch reads, where
/// the executor's LDS stage of the window starts; dst high word = Rv: the
/// rows [0, Rv) that may read versioned sums, kVersionRows at most, 0 when no
/// update of the batch joined after a row read its sum):
///   24 words   WinEntry of the lane sums as the rows read them (lane*3 + s)
///   E words    WinEntry of window elements [base, base+E): an absent
///              (lost) element has len 0 and contributes nothing
///   U words    SumUpdate, run before any row of the batch (no row of the
///              batch reads a sum updated in it before the update; ops.h
///              invariant kept by Program)
///   R*3 words  RowItem
struct WinEntry
{
    uint64_t src;
    uint32_t len;
    uint32_t column;     // packet number (selects CX for sum updates)
};

/// dst[0,n) = keep(dst,valid) ^ sum over elements e = from, from+8, ... < to
/// of coeff(e) * window[e], coeff = 1, CX(column) or CX(column)^2 (s = 0..2).
struct SumUpdate
{
    uint32_t dstLo, dstHi;
    uint32_t n;
    uint32_t valid : 30;
    uint32_t s : 2;
    uint32_t from;
    uint32_t to;
    uint32_t sum;        // which of the 24 lane sums the rows read (lane*3+s) dst is
    uint32_t pad;
};

/// One Siamese row: dst[0,n) = keep(dst,valid) ^ acc0 ^ mix*acc1 where
///   acc0 = sums selected by mask0 (bit lane*3+s) ^ window[ldpcOff + PCG_2i % ldpcN]
///   acc1 = sums selected by mask1              ^ window[ldpcOff + PCG_2i+1 % ldpcN]
/// over i < ceil(ldpcN/16) pairs of PCG.Seed(row, ldpcN) draws, then litLen
/// footer bytes at dst + n.
///
/// A row reads each sum as it stood when the row was made: the batch's sum
/// updates are incremental (each extends its sum over later window elements,
/// SumUpdate), so sum k as row r reads it is the sum after every update of
/// the batch with the contributions of the update's elements at or past the
/// row's `cutoff` (batch-relative element index) taken back out.  Rows made
/// one after another in a streaming encoder (each folding the originals
/// added since the previous one into the sums it reads) then share one batch
/// instead of a batch each.  A batch with such joins (Program::rows_update)
/// holds at most kVersionRows rows, and only short joins: the executor
/// computes the corrections of each (row, lane) pair in parallel.
constexpr unsigned kVersionRows = 16;
constexpr unsigned kVersionMaxSpan = 32;   // window elements one joining update may add
struct RowItem
{
    uint64_t dst;
    uint32_t n;
    uint32_t valid;
    uint32_t mask0;      // bits 0..23; bits 24..30: litLen; bit 31: kRowWide
    uint32_t mask1;      // bits 0..23; bits 24..31: mix (RX)
    uint32_t row;
    uint32_t ldpcN;
    uint32_t ldpcOff;
    uint32_t cutoff;     // sums as of window elements < cutoff (batch-relative)
    uint8_t lit[8];
};
/// RowItem.mask0 bit 31: a wide row whose LDPC sums k_ldpc computed
/// (LdpcItem): ldpcN = 0, and window entries ldpcOff / ldpcOff + 1 hold L0 /
/// L1, added to acc0 / acc1 as two draws would be.
constexpr uint32_t kRowWide = 1u << 31;
inline constexpr uint32_t row_lit_len(uint32_t mask0) { return (mask0 >> 24) & 0x7fu; }
static_assert(sizeof(WinEntry) == 16, "WinEntry layout");
static_assert(sizeof(SumUpdate) == 32, "SumUpdate layout");
static_assert(sizeof(RowItem) == 48, "RowItem layout");
constexpr unsigned kRowSums = 24;                       // kLanes * kSums
constexpr unsigned kUpdateWords = sizeof(SumUpdate) / 16;
constexpr unsigned kRowWords = sizeof(RowItem) / 16;
/// Words of an OP_ROWS block the executor keeps in its LDS table: the 24 sum
/// entries, then the block's words from window element stageLo on.  A batch
/// whose block, less the stageLo entries it skips, is longer reads the rest
/// from the stream (Engine counts those batches, sgpu_engine_stats_ex [33]).
constexpr unsigned kRowsTableLds = 1024;

/// Wide rows (ldpcN >= kLdpcSplitMin): the O(window) LDPC part of a row is
/// too much for the one workgroup per tile that runs the codec's op list, so
/// k_ldpc computes it first, spread over the whole chip: item k covers pairs
/// [pair0, pair1) of PCG.Seed(row, N) on one 1 KiB tile and XORs
///   L0 = sum of the even draws' window elements  into dst[0, n)
///   L1 = sum of the odd draws' window elements   into dst[span, span + n)
/// (a zeroed scratch area; items of one row meet by atomic XOR).  The row in
/// the OP_ROWS block then carries kRowWide, ldpcN = 0 and ldpcOff = the
/// window index of two entries appended to the batch's window that name L0
/// and L1, and adds them to acc0 and acc1 like two draws.  The same bytes
/// meet in a different order, which GF(2^8) addition (XOR) does not see.
///
/// Gated items (a chained decode's wide rows, GeDesc kGeChained): LdpcItem has
/// no spare field, so a launch that holds gated items takes a parallel array
/// of one gate word per item, 0 or 1 + a result word as GfOp.termBegin: the
/// item does nothing (writes nothing, counts nothing) when that word is zero,
/// its scratch pair stays zero, and the kRowWide row that would read it lies
/// in the same gated OP_ROWS op.  Launches without gated items take no array
/// and run the ungated instantiation of the kernel.
struct LdpcItem
{
    uint64_t win;        // device address of the batch's window entry 0 (WinEntry[])
    uint64_t dst;        // L0 at dst, L1 at dst + span
    uint32_t span;
    uint32_t n;          // row bytes
    uint32_t row;
    uint32_t N;          // PCG.Seed(row, N); element = off + draw % N
    uint32_t off;
    uint32_t tileBase;
    uint32_t pair0, pair1;
};
static_assert(sizeof(LdpcItem) == 48, "LdpcItem layout");
constexpr uint32_t kLdpcSplitMin = 512;      // ldpcN from which a row's picks go to k_ldpc
#ifndef SGPU_LDPC_PAIRS
#define SGPU_LDPC_PAIRS 64
#endif
constexpr uint32_t kLdpcTileBytes = 1024;    // k_ldpc tile: 64 lanes x 16 bytes
/// Pairs per k_ldpc item for a row of `bytes`: rows of large symbols (C5:
/// 64 tiles each) take SGPU_LDPC_PAIRS, which halves their atomics and item
/// count (C5 66-69 ms/run vs 68-81 with 32); rows of small symbols keep 32,
/// so their few tiles still spread over enough workgroups (C3: k_ldpc 10.3
/// vs 13.1 us per launch with 64).  profiles/r3g_ldpc_item_ab.txt, r3h traces.
constexpr uint32_t ldpc_pairs_per_item(uint32_t bytes)
{
    return bytes >= 16 * kLdpcTileBytes ? SGPU_LDPC_PAIRS : 32u;
}

/// OP_COPIES: n independent copies (the decoder taking in recovery packets,
/// reference SiameseDecoder.cpp:437), one CopyItem word pair each after the
/// GfOp header (termCount = 2n).  dst[0,len) = src[0,len) with the zero tail
/// of every write; copies of one batch never overlap, so the executor deals
/// them to its waves without barriers.
struct CopyItem
{
    uint64_t dst;
    uint64_t src;
    uint32_t len;
    uint32_t pad[3];
};
static_assert(sizeof(CopyItem) == 32, "CopyItem layout");
constexpr unsigned kCopyWords = sizeof(CopyItem) / 16;

/// OP_LINCOMBS: n mutually independent linear combinations (no item reads or
/// writes bytes another item of the batch writes), each optionally followed
/// by a literal (a recovery packet's footer) on its own dst.  After the GfOp
/// header (termCount = the block's words): n LcItem (3 words each), then the
/// items' GfTerm words; termStart is an item's first term word within the
/// block.  The executor gives each wave whole items, so a run of small
/// combinations (Cauchy / parity rows of a short window, reference
/// SiameseEncoder.cpp:1334-1441, and the decoder's elimination of received
/// originals from each recovery packet, SiameseDecoder.cpp:812-1063) costs
/// one memory round trip and one barrier instead of one per combination.
struct LcItem
{
    uint64_t dst;
    uint32_t n, valid;           // as OP_LINCOMB
    uint32_t termStart, termCount;
    uint32_t mixLit;             // mix | litLen << 8
    uint32_t litOffset;          // literal at dst + litOffset (litLen <= 8)
    uint8_t lit[8];
    uint32_t pad[2];
};
static_assert(sizeof(LcItem) == 48, "LcItem layout");
constexpr unsigned kLcWords = sizeof(LcItem) / 16;
constexpr unsigned kLcMaxTerms = 64;    // larger combinations keep all waves on one op
constexpr unsigned kLcMaxItems = 256;

/// PCG-XSH-RR as the reference seeds it (SiameseTools.h:80-102).
constexpr uint64_t kPcgMul = 6364136223846793005ULL;

inline uint32_t op_words(const GfOp& op)
{
    // (an OP_ROWS header's termCount is its whole block in words)
    return kOpWords +
           ((op.kind == OP_LINCOMB || op.kind == OP_ROWS || op.kind == OP_COPIES || op.kind == OP_LINCOMBS)
                ? op.termCount
                : 0);
}

/// Executor work item: one (instance segment, byte tile).
struct ExecItem
{
    uint32_t streamBegin;  // first 16-byte word of the segment's stream
    uint32_t streamWords;  // words in the segment's stream
    uint32_t opCount;
    uint32_t tiles;        // exec_tiles(first 256-byte tile, tile count): the workgroup runs
                           // the op list over each tile (op by op, every tile in turn)
};
/// ExecItem.tiles: the first tile in the low 24 bits (16M tiles of 256 B:
/// 4 GiB, past SIAMESE_MAX_PACKET_BYTES), the run's tile count (1..255) in
/// the high 8.
constexpr uint32_t kExecRunMax = 255;
constexpr uint32_t kExecFirstTileMask = 0xffffffu;
constexpr uint32_t exec_tiles(uint32_t firstTile, uint32_t count) { return firstTile | count << 24; }
constexpr uint32_t exec_first_tile(uint32_t tiles) { return tiles & kExecFirstTileMask; }
constexpr uint32_t exec_tile_count(uint32_t tiles) { return tiles >> 24; }

/// Triangular solve of one decode (reference SiameseDecoder.cpp:1065-1238).
/// Rows are listed in pivot order; coef is an m x m byte matrix with
/// coef[j*m + i] = RecoveryMatrix[Pivots[j]][i].
struct SolveDesc
{
    uint32_t m;
    uint32_t rowBegin;   // index into SolveRow array
    uint64_t coefOffset; // byte offset into coefficient array
    uint32_t result;     // index into the uint32 result array (m+2 words:
                         // [0] rows recovered, [1..m] lengths, [m+1] set
                         // when a product solve's rows have non-zero bytes
                         // past their recovered lengths)
    uint32_t maxBytes;   // max finalBytes over rows (tile count)
    uint64_t head;       // m x 16 bytes: each row's first 16 bytes as the solve
                         // starts (copied by the segment before it), so every
                         // tile can solve the length prefixes while tile 0
                         // overwrites the rows
    uint64_t tinv;       // device scratch of solve_t_bytes(m) for the solve's
                         // inverse T (product solves; 0: none)
    uint64_t xout;       // device scratch of solve_x_bytes(m, maxBytes): the
                         // product solves' result rows, copied into the rows
                         // by the tile pass unless the solve is flagged (the
                         // rows keep their inputs for the exact sweeps)
    uint32_t gate;       // 0, or 1 + a result word: the solve runs only if that
                         // word is non-zero (a chained device elimination's
                         // outcome, GeDesc kGeChained: its rows and
                         // coefficients are what k_ge wrote)
    uint32_t pad;
};

/// Solves of up to this many rows may run as the product X = T R (their
/// inverse T = U^-1 L^-1 in scratch, rows of kTStride bytes), in split
/// launches (solve_split: the prefix pass is then its own launch).
constexpr unsigned kProductMaxRows = 120;
constexpr unsigned kSolvePrefixSplit = 16;
constexpr unsigned kSolveSplitMinRows = 16;
/// Whether a launch's solves take the split form (prefix pass and inverse,
/// product, copy-in: three launches) rather than k_solve_main's fused sweeps:
/// many solves, or any solve whose serial sweeps would outlast the three
/// launches (a lone 51-row solve: 209 us as sweeps, profiles/r6_kernel_stats).
constexpr bool solve_split(uint32_t solveCount, uint32_t maxRows)
{
    return solveCount >= kSolvePrefixSplit || maxRows >= kSolveSplitMinRows;
}
constexpr uint32_t kTStride = 128;
constexpr uint32_t solve_t_bytes(uint32_t m)
{
    return m <= kProductMaxRows ? ((m + 3u) & ~3u) * kTStride : 0u;
}
/// Row stride of the product solves' result scratch (64-byte chunks).
constexpr uint32_t solve_x_stride(uint32_t maxBytes) { return (maxBytes + 63u) & ~63u; }
constexpr uint64_t solve_x_bytes(uint32_t m, uint32_t maxBytes)
{
    return m <= kProductMaxRows ? (uint64_t)m * solve_x_stride(maxBytes) : 0u;
}

struct SolveRow
{
    uint64_t buf;        // recovery buffer (becomes the recovered original)
    uint32_t initBytes;  // Bytes before MultiplyLowerTriangle
    uint32_t lowerLen;   // Bytes when this row is the source of the lower step
    uint32_t finalBytes; // Bytes after MultiplyLowerTriangle
    uint32_t headIndex;  // 1 + the row's slot in SolveDesc.head (0: its own
                         // index; a chained elimination permutes the rows into
                         // pivot order after their heads were laid out)
};
constexpr uint32_t solve_head_slot(uint32_t headIndex, uint32_t j) { return headIndex ? headIndex - 1u : j; }

/// Result word layout for each recovered row: (headerBytes << 29) | length,
/// or 0 if the prefix failed validation.  Word 0 holds the number of rows
/// recovered before the first invalid one (== m when all are valid), counting
/// from the right-most column as the reference does.
constexpr uint32_t kSolveLengthMask = 0x1fffffffu;

/// Solve work item: one (solve, byte tile).
struct SolveItem
{
    uint32_t solve;
    uint32_t tileBase;
};

/// Ingest of a run of `count` symbols into FRESH device buffers (never
/// referenced by any op of the same flush before this point), so ingest can
/// run as the first launch of a flush.  Symbol k of the run (k < count; a
/// count of 0 reads as 1) has its source at src + k * srcStride and its
/// destination at dst + k * dstStride:  dst[0,hdrLen) = hdr,
/// dst[hdrLen, hdrLen+bytes) = src, and dst[total, align16(total)) = 0 (whole
/// 16-byte lanes are stored; dst is 16-byte aligned with capacity >=
/// align16(total)).  Bit k of dst2Mask set: symbol k is also written to the
/// fresh buffer dst2 + k * dstStride (an encoder and a decoder ingesting the
/// same originals: the source is read once; the decoder's lost originals
/// are the clear bits).  A run is a slab's consecutive slots filled from
/// consecutive device originals: one descriptor instead of one per symbol.
struct IngestDesc
{
    uint64_t dst;
    uint64_t src;
    uint64_t dst2;
    uint64_t dst2Mask;
    uint32_t bytes;
    uint32_t hdrLen;
    uint8_t hdr[8];
    uint32_t count;
    uint32_t srcStride;
    uint32_t dstStride;
    uint32_t pad;
};

/// Symbols of one ingest run at most (k_ingest block table: 4 bits of
/// 4-symbol groups per entry).
constexpr uint32_t kIngestRunMax = 64;
/// k_ingest work per workgroup: one symbol per wave.
constexpr uint32_t kIngestWaves = 4;

/// Delivery of one decoder packet into caller-owned device memory (k_deliver,
/// sgpu_decoder_deliver_range): k_ingest run backwards.  The symbol at src
/// (16-byte aligned, its 1-4 byte length prefix at byte 0) is read on the
/// device: header h and length L from the prefix (reference
/// SiameseSerializers.h:598-640), valid when L >= 1, h + L <= cap and
/// L <= stride.  Then dst[0, L) = src[h, h + L), dst[L, stride) = 0 and
/// *lenOut = L; an invalid packet counts as L = 0 (a zeroed row).  src = 0: an
/// absent packet, only *lenOut = 0 is written.  Only aligned 16-byte words
/// holding a byte of [src, src + cap) are read, nothing outside
/// [dst, dst + stride) and the length word is written.  The launch runs after
/// every other launch of its submission, so the prefix of a packet whose solve
/// rides in the same submission is already in place.
struct DeliverItem
{
    uint64_t src;        // the symbol (0: absent)
    uint64_t dst;        // the row, 16-byte aligned
    uint64_t lenOut;     // uint32 length word, 4-byte aligned
    uint32_t cap;        // bytes of the symbol that may be read: header + length
                         // of a received packet, finalBytes of a pending row
    uint32_t stride16;   // the row's bytes / 16 (1 .. 2^28: rows of up to 4 GiB)
};
static_assert(sizeof(DeliverItem) == 32, "DeliverItem layout");
/// k_deliver work per workgroup: one item per wave, as k_ingest; a wave takes
/// the kIngestChunkBytes chunks blockIdx.y, blockIdx.y + gridDim.y, ... of its
/// row, and a launch has at most kDeliverMaxChunks chunk rows in its grid.
constexpr uint32_t kDeliverWaves = 4;
constexpr uint32_t kDeliverMaxChunks = 4096;

/// One sender packet framed into a caller-owned device row (k_frame,
/// sgpu_frames_deliver_recovery / sgpu_encoder_deliver_range).  With
/// T = hdrLen + bytes:  dst[0, hdrLen) = hdr, dst[hdrLen, T) = src[0, bytes),
/// dst[T, stride) = 0 and *lenOut = lenBase + T (the host guarantees T <= stride).  src
/// has any byte alignment (a recovery packet's arena buffer, or an original's
/// slot address plus its prefix bytes); src = 0: an absent packet, only
/// *lenOut = lenBase is written.  lenOut = 0: no length word is written (a
/// frame that is not the last of a packed row, sgpu_encoder_pack_frames, where
/// dst is the frame's slot in the row, stride16 the slot's span and lenBase the
/// slot's offset in the row).  Only aligned 16-byte words holding a byte of
/// [src, src + bytes) are read, nothing outside [dst, dst + stride) and the
/// length word is written.  hdr is the literal frame header (frames.h: an
/// original's is prefix <= 4 plus 7 bytes), hdrLen = 0 for a bare packet.  The
/// launch runs after every other launch of its submission, beside k_deliver.
constexpr unsigned kFrameMaxHeader = 11;
constexpr unsigned kFrameMaxLength = 0x1fffffff;   // the largest L a frame's 4-byte length prefix holds
struct FrameItem
{
    uint64_t src;        // the packet's first byte (0: absent)
    uint64_t dst;        // the row, 16-byte aligned
    uint64_t lenOut;     // uint32 length word, 4-byte aligned (0: none)
    uint32_t bytes;      // packet bytes after the header
    uint32_t stride16;   // the row's bytes / 16 (1 .. 2^28)
    uint8_t hdr[kFrameMaxHeader];
    uint8_t hdrLen;
    uint32_t lenBase;    // added to the length word (0 but for a packed row's last frame)
};
static_assert(sizeof(FrameItem) == 48, "FrameItem layout");
/// k_frame's grid is k_deliver's: kDeliverWaves items per workgroup, at most
/// kDeliverMaxChunks chunk rows.

/// One decoder packet forwarded as an original's wire frame into a
/// caller-owned device row (k_relay, sgpu_decoder_deliver_frames): DeliverItem
/// with the frame header computed on the device from the length it reads.  The
/// symbol at src (16-byte aligned, its 1-4 byte length prefix at byte 0) gives
/// its header hs and length n as for k_deliver; the frame header of an original
/// of n bytes for `flow` and `packetNum` (frames.h frame_write_header) has hf =
/// 8..11 bytes.  Valid when n >= 1, hs + n <= cap and hf + n <= stride: then
/// dst[0, hf) = that header, dst[hf, hf + n) = src[hs, hs + n),
/// dst[hf + n, stride) = 0 and *lenOut = hf + n; an invalid packet gets a zeroed
/// row and *lenOut = 0.  src = 0: an absent packet, only *lenOut = 0 is written.
/// Only aligned 16-byte words holding a byte of [src, src + cap) are read,
/// nothing outside [dst, dst + stride) and the length word is written
/// (frames.h relay_row states the row in plain C++).  The launch runs after
/// every other launch of its submission, beside k_deliver and k_frame.
struct RelayItem
{
    uint64_t src;        // the symbol (0: absent)
    uint64_t dst;        // the row, 16-byte aligned
    uint64_t lenOut;     // uint32 length word, 4-byte aligned
    uint32_t cap;        // as DeliverItem.cap
    uint32_t stride16;   // the row's bytes / 16 (1 .. 2^28)
    uint32_t flow;       // the frame's flow (<= 2^24 - 1)
    uint32_t packetNum;  // the frame's PacketNum
};
static_assert(sizeof(RelayItem) == 40, "RelayItem layout");
/// k_relay's grid is k_deliver's too.

/// A decoder's packets forwarded as originals' wire frames, several to a row
/// (k_plan and k_pack, sgpu_decoder_pack_frames).  One PackJob per call, one
/// PackItem per packet of its range, in packet order; k_plan writes one PlanRec
/// per item into scratch of the submission, k_pack reads it.
///
/// An item's frame is RelayItem's: hs, n and hf from the symbol's first bytes,
/// T = hf + n when it fits (frames.h relay_fits, with the job's stride), T = 0
/// for an absent packet (src = 0) or one that does not fit.  k_plan walks the
/// packer's cursor rule over the job's T in item order (frames.h pack_plan: a
/// frame with off + T > stride opens the next row, is placed at off, and off
/// becomes align16(off + T)) and gives every frame its row, its offset and its
/// span: the bytes up to the next frame of the row, or to the row's end.  It
/// writes the job's maxRows length words (the end of the row's last frame; zero
/// for a row without one) and info = {rows needed, frames written, present
/// packets that do not fit, frames dropped because row >= maxRows}.  k_pack
/// writes dst[0, span) of every frame flagged kPlanWrite, dst = rows +
/// row * stride + 16 * off16, as relay_row writes a row of span bytes.  Nothing
/// else is written; only aligned 16-byte words holding a byte of
/// [src, src + cap) are read.
struct PackItem
{
    uint64_t src;        // the symbol (0: absent)
    uint32_t cap;        // as DeliverItem.cap
    uint32_t flow;       // the frame's flow (<= 2^24 - 1)
    uint32_t packetNum;  // the frame's PacketNum
    uint32_t job;        // index of the item's PackJob in the launch
};
static_assert(sizeof(PackItem) == 24, "PackItem layout");
struct PackJob
{
    uint64_t rows;       // row 0, 16-byte aligned (not read when maxRows = 0)
    uint64_t lens;       // maxRows uint32 length words, 4-byte aligned
    uint64_t info;       // four uint32, 16-byte aligned
    uint32_t first;      // index of the job's first item in the launch
    uint32_t count;      // its items (<= 65535)
    uint32_t stride16;   // a row's bytes / 16 (1 .. 2^28)
    uint32_t maxRows;    // rows and length words the caller owns
};
static_assert(sizeof(PackJob) == 40, "PackJob layout");
struct PlanRec
{
    uint32_t row;        // the frame's row
    uint32_t off16;      // its offset in the row / 16
    uint32_t span16;     // bytes to the next frame of the row or to the row's end, / 16
    uint32_t flags;      // kPlanWrite, or 0: not a frame, or a frame of a row >= maxRows
};
static_assert(sizeof(PlanRec) == 16, "PlanRec layout");
constexpr uint32_t kPlanWrite = 1;
constexpr uint32_t kPackMaxItems = 65535;   // items of one job
/// k_plan runs one wave per job, kDeliverWaves jobs per workgroup; k_pack's
/// grid is k_deliver's over the items, the chunk rows sized by the longest
/// stride (a span is at most a row).

/// A decoder's packets as one contiguous byte stream (k_offsets and k_concat,
/// sgpu_decoder_deliver_stream).  One ConcatJob per call, one ConcatItem per
/// packet of the range's leading present run (count = p of them; the range has
/// `total` packets), in packet order; k_offsets writes one ConcatRec per item
/// into scratch of the submission, k_concat reads it.
///
/// An item's payload is DeliverItem's: hs and n from the symbol's first bytes,
/// valid when n >= 1 and hs + n <= cap.  k_offsets sums the job's n in item
/// order (frames.h concat_plan): off_0 = 0, item k is delivered when every item
/// before it was, it is valid and off_k + n <= capacity, and then off_{k+1} =
/// off_k + n.  With d items delivered and B = off_d it writes the job's
/// total + 1 offset words (off_k for k <= d, B behind) and info = {d, B, stop,
/// count}, stop 0 for d == count, 1 for an invalid item d, 2 for one that does
/// not fit.  k_concat writes dst[off, off + n) = src[hs, hs + n) of every record
/// flagged kConcatWrite, dst at any byte alignment, and no other byte: words
/// that two neighbouring packets share are written by byte-granular stores and
/// never read.  Only aligned 16-byte words holding a byte of [src, src + cap)
/// are read.
struct ConcatItem
{
    uint64_t src;        // the symbol, 16-byte aligned (never 0: only present packets are items)
    uint32_t cap;        // as DeliverItem.cap
    uint32_t job;        // index of the item's ConcatJob in the launch
};
static_assert(sizeof(ConcatItem) == 16, "ConcatItem layout");
struct ConcatJob
{
    uint64_t dst;        // the stream's byte 0, any alignment (not read when capacity = 0)
    uint64_t offsets;    // total + 1 uint32 offset words, 4-byte aligned
    uint64_t info;       // four uint32, 16-byte aligned
    uint32_t capacity;   // bytes the caller owns at dst
    uint32_t first;      // index of the job's first item in the launch
    uint32_t count;      // its items (<= total)
    uint32_t total;      // packets of the call's range (<= 65535)
};
static_assert(sizeof(ConcatJob) == 40, "ConcatJob layout");
struct ConcatRec
{
    uint32_t off;        // the payload's offset in the stream
    uint32_t n;          // its bytes
    uint32_t hs;         // the symbol's prefix bytes (1..4)
    uint32_t flags;      // kConcatWrite, or 0: not delivered
};
static_assert(sizeof(ConcatRec) == 16, "ConcatRec layout");
constexpr uint32_t kConcatWrite = 1;
constexpr uint32_t kConcatMaxItems = 65535;   // packets of one job
/// k_offsets runs one wave per job, kDeliverWaves jobs per workgroup; k_concat's
/// grid is k_deliver's over the items, the chunk rows sized by the longest
/// symbol (a payload is shorter than its symbol).

/// What the host needs of one frame row that lives in device memory (k_scan,
/// sgpu_frames_scan_rows): the layout of SgpuRowHead (include/siamese_gpu.h),
/// written as eight dwords
///   [0] frameBytes  [1] status | type << 8 | headerBytes << 16 | tailBytes << 24
///   [2] flow  [3] packetNum  [4] dataBytes  [5] head  [6..7] tail.
/// Row k starts at rows + k * stride (16-byte aligned, stride a multiple of
/// 16).  With a length array, lens[k] == 0 makes the row empty and a non-zero
/// word must equal the frame's prefix + L; without one a zero first byte does.
/// Otherwise the row's first 16 bytes are parsed as a frame header (frames.h)
/// and checked (frames.h row_head_valid states the checks); a recovery row
/// also gives its first min(4, dataBytes) bytes (head) and its last
/// tailBytes = min(8, dataBytes) bytes, right-aligned in tail.  An empty or
/// malformed record is zero but for its status.  Nothing outside
/// [row, row + stride) and the row's length word is read.
constexpr uint8_t kRowEmpty = 0, kRowOk = 1, kRowMalformed = 2;
struct RowHead
{
    uint32_t frameBytes;   // prefix + L (0: empty or malformed)
    uint8_t status;        // kRowEmpty / kRowOk / kRowMalformed
    uint8_t type;          // kFrameOriginal / kFrameRecovery
    uint8_t headerBytes;   // offset of the data in the row (<= kFrameMaxHeader)
    uint8_t tailBytes;
    uint32_t flow;
    uint32_t packetNum;    // originals
    uint32_t dataBytes;
    uint8_t head[4];
    uint8_t tail[8];
};
static_assert(sizeof(RowHead) == 32, "RowHead layout");
/// k_scan: one lane per row, kScanThreads rows per workgroup.
constexpr uint32_t kScanThreads = 256;

/// One frame of a row that holds several (k_walk, sgpu_frames_scan_packed):
/// the layout of SgpuPackedHead, RowHead with the frame's offset in the row in
/// place of frameBytes; the data is at offset + headerBytes.  Row k of a scan
/// with maxFrames records per row owns records [k * maxFrames, (k + 1) *
/// maxFrames) and, after all records, row word k: the number of records that
/// are kRowOk (the row's first ones; the rest are zero) with kPackedMore when
/// a non-zero byte is left after maxFrames frames and kPackedMalformed when
/// the walk stopped at a frame it could not accept (frames.h row_walk states
/// the walk).  Nothing outside [row, row + stride) and the row's length word
/// is read.
struct PackedHead
{
    uint32_t offset;       // of the frame's length prefix in the row
    uint8_t status;        // kRowEmpty / kRowOk
    uint8_t type;
    uint8_t headerBytes;   // prefix + inner header (<= kFrameMaxHeader)
    uint8_t tailBytes;
    uint32_t flow;
    uint32_t packetNum;
    uint32_t dataBytes;
    uint8_t head[4];
    uint8_t tail[8];
};
static_assert(sizeof(PackedHead) == 32, "PackedHead layout");
constexpr uint32_t kPackedMore = 0x80000000u, kPackedMalformed = 0x40000000u, kPackedCountMask = 0xffffu;
constexpr uint32_t kPackedMaxFrames = 256;
/// k_walk: one lane per row, kWalkThreads rows per workgroup.
constexpr uint32_t kWalkThreads = 256;
/// Bytes of a packed scan's output: the records, then the row words.
constexpr uint64_t packed_bytes(uint64_t count, uint64_t maxFrames)
{
    return count * maxFrames * sizeof(PackedHead) + count * 4;
}

/// Rows of a bidirectional flow (k_ackwalk, sgpu_frames_scan_duplex): k_walk's
/// records and row words, with acknowledgement frames (frames.h kFrameAck)
/// accepted, and behind the row words, from the next 16-byte boundary on,
/// ackSlots message slots of ackBytes bytes per row (row k's at slot index
/// k * ackSlots).  The row's a-th ack frame, of D message bytes, gets a record
/// with type kFrameAck, packetNum = a, dataBytes = D, no head and no tail; when
/// a < ackSlots, slot a holds the message's first min(D, ackBytes) bytes and
/// zeros after them.  Its status is kRowOk when a < ackSlots and D <= ackBytes,
/// otherwise kRowTruncated, and the row word then carries kPackedAcksDropped:
/// the walk goes on either way.  Slots without an ack are zero (frames.h
/// ack_walk states the walk).
constexpr uint8_t kRowTruncated = 3;
constexpr uint32_t kPackedAcksDropped = 0x20000000u;
constexpr uint32_t kAckSlotBytesMin = 16, kAckSlotBytesMax = 1024;   // ackBytes: a multiple of 16 between them
/// k_ackwalk: one lane per row, kAckWalkThreads rows per workgroup.
constexpr uint32_t kAckWalkThreads = 256;
/// Where a duplex scan's slots start, and its output's bytes.
constexpr uint64_t duplex_slots_offset(uint64_t count, uint64_t maxFrames)
{
    return (packed_bytes(count, maxFrames) + 15) & ~(uint64_t)15;
}
constexpr uint64_t duplex_bytes(uint64_t count, uint64_t maxFrames, uint64_t ackSlots, uint64_t ackBytes)
{
    return duplex_slots_offset(count, maxFrames) + count * ackSlots * ackBytes;
}

/// The packed scan's records without the empty slots (k_walkd, k_rowsum and
/// k_compact, sgpu_frames_scan_dense): the accepted records of all rows back to
/// back in row order, behind a table of per-row start indices.  The output is
///   info {T, W, c, 0} | count row words | count + 1 start words | zeros to the
///   next 16-byte boundary | maxRecords PackedHead records
/// where row word k is k_walk's, n_k its count, start[0] = 0, start[k + 1] =
/// start[k] + n_k, T = start[count], c the largest value with start[c] <=
/// maxRecords and W = start[c].  Records [start[k], start[k + 1]) for k < c are
/// row k's first n_k records as k_walk writes them (offset relative to the row);
/// records [W, maxRecords) are zero (frames.h dense_compact states all of it).
/// maxFrames <= maxRecords <= count * maxFrames, so c >= 1 for count >= 1.
///
/// On the device the walk writes each row's records into a scratch area of
/// count * maxFrames records behind the output (dense_scratch_offset), which
/// never crosses to the host.  k_rowsum is one workgroup of kRowsumThreads
/// lanes that strides over the rows, kRowsumRows consecutive rows per lane and
/// so kRowsumPass rows per pass; k_compact takes one record slot per pair of
/// lanes, kCompactThreads lanes per workgroup.
constexpr uint32_t kRowsumThreads = 1024;
constexpr uint32_t kRowsumRows = 8;
constexpr uint32_t kRowsumPass = kRowsumThreads * kRowsumRows;
constexpr uint32_t kCompactThreads = 256;
/// Where a dense scan's records start, its output's bytes, and where the
/// device's scratch records start in the staging area.
constexpr uint64_t dense_records_offset(uint64_t count)
{
    return (16 + count * 4 + (count + 1) * 4 + 15) & ~(uint64_t)15;
}
constexpr uint64_t dense_bytes(uint64_t count, uint64_t maxRecords)
{
    return dense_records_offset(count) + maxRecords * sizeof(PackedHead);
}
constexpr uint64_t dense_scratch_offset(uint64_t count, uint64_t maxRecords)
{
    return dense_bytes(count, maxRecords);   // (a multiple of 16)
}
constexpr uint64_t dense_stage_bytes(uint64_t count, uint64_t maxFrames, uint64_t maxRecords)
{
    return dense_scratch_offset(count, maxRecords) + count * maxFrames * sizeof(PackedHead);
}

/// The duplex scan in dense form (k_ackwalkd, k_rowsum2, k_compact and k_slots,
/// sgpu_frames_scan_duplex_dense): the dense layout above with info word 3 =
/// WA, and behind the records a second table and the acks' message slots back
/// to back.  The output is
///   info {T, W, c, WA} | count row words | count + 1 start words | zeros to the
///   next 16-byte boundary | maxRecords PackedHead records | count + 1 ack start
///   words | zeros to the next 16-byte boundary | maxAcks slots of ackBytes
/// where row word k is k_ackwalk's, a_k = min(ack frames of row k, ackSlots),
/// astart[0] = 0 and astart[k + 1] = astart[k] + a_k.  Rows are all or nothing
/// over both budgets: c is the largest value with start[c] <= maxRecords and
/// astart[c] <= maxAcks, W = start[c], WA = astart[c].  Slot astart[k] + a, for
/// k < c and a < a_k, is row k's slot a as k_ackwalk writes it; slots [WA,
/// maxAcks) are zero (frames.h duplex_dense_compact states all of it).
/// ackSlots <= maxAcks <= count * ackSlots.
///
/// On the device the walk writes into scratch areas behind the output, none of
/// which crosses to the host: count * maxFrames records, count * ackSlots slots
/// and count ack counts.  Every offset below is a multiple of 16.  k_ackwalkd
/// takes one lane per row, kAckWalkdThreads rows per workgroup; k_rowsum2 is
/// k_rowsum's single striding workgroup (kRowsum2Threads lanes, kRowsum2Rows
/// consecutive rows per lane, kRowsum2Pass rows per pass) over both counts at
/// once; k_slots takes one 16-byte word of the slot area per lane, kSlotsThreads
/// lanes per workgroup.
constexpr uint32_t kAckWalkdThreads = 256;
constexpr uint32_t kRowsum2Threads = 1024;
constexpr uint32_t kRowsum2Rows = 8;
constexpr uint32_t kRowsum2Pass = kRowsum2Threads * kRowsum2Rows;
constexpr uint32_t kSlotsThreads = 256;
/// Where a duplex dense scan's ack starts and slots begin, and its output's bytes.
constexpr uint64_t duplex_dense_acks_offset(uint64_t count, uint64_t maxRecords)
{
    return dense_bytes(count, maxRecords);   // (a multiple of 16)
}
constexpr uint64_t duplex_dense_slots_offset(uint64_t count, uint64_t maxRecords)
{
    return duplex_dense_acks_offset(count, maxRecords) + (((count + 1) * 4 + 15) & ~(uint64_t)15);
}
constexpr uint64_t duplex_dense_bytes(uint64_t count, uint64_t maxRecords, uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_dense_slots_offset(count, maxRecords) + maxAcks * ackBytes;   // (ackBytes: a multiple of 16)
}
/// The device's scratch areas in the staging area: the rows' records, the rows'
/// slots, the rows' ack counts (rounded up to whole 16-byte words).
constexpr uint64_t duplex_dense_scratch_records(uint64_t count, uint64_t maxRecords, uint64_t maxAcks,
                                                uint64_t ackBytes)
{
    return duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes);
}
constexpr uint64_t duplex_dense_scratch_slots(uint64_t count, uint64_t maxFrames, uint64_t maxRecords,
                                              uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_dense_scratch_records(count, maxRecords, maxAcks, ackBytes) + count * maxFrames * sizeof(PackedHead);
}
constexpr uint64_t duplex_dense_scratch_counts(uint64_t count, uint64_t maxFrames, uint64_t ackSlots,
                                               uint64_t maxRecords, uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_dense_scratch_slots(count, maxFrames, maxRecords, maxAcks, ackBytes) + count * ackSlots * ackBytes;
}
constexpr uint64_t duplex_dense_stage_bytes(uint64_t count, uint64_t maxFrames, uint64_t ackSlots,
                                            uint64_t maxRecords, uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_dense_scratch_counts(count, maxFrames, ackSlots, maxRecords, maxAcks, ackBytes) +
           ((count * 4 + 15) & ~(uint64_t)15);
}

/// Byte-stream rows (k_streamwalk, k_rowsum and k_compact,
/// sgpu_frames_scan_streams): row k is a connection's receive buffer whose bytes
/// [start_k, end_k) hold frames back to back, the last of which may still be
/// arriving.  The output is the dense layout above (dense_bytes) and behind it
///   count next words | zeros to the next 16-byte boundary
/// where row word k may carry kStreamPartial (the walk stopped at a frame the
/// data does not yet hold whole) and next_k is the row offset from which the
/// row's next scan must start (frames.h stream_walk states the walk).  A
/// record's offset is relative to the row's first byte, not to start_k.
///
/// On the device the walk takes one wave per row, kStreamWalkThreads / 64 rows
/// per workgroup, and consumes the row in chunks of kStreamChunk bytes (64 lanes
/// x 16 bytes) staged in LDS with a 16-byte halo; its per-row scratch records lie
/// behind the output as the dense scan's do (streams_scratch_offset).
constexpr uint32_t kStreamPartial = 0x20000000u;
constexpr uint32_t kStreamChunk = 1024;
constexpr uint32_t kStreamWalkThreads = 256;
/// Where a stream scan's next words start, its output's bytes, and where the
/// device's scratch records start in the staging area.
constexpr uint64_t streams_next_offset(uint64_t count, uint64_t maxRecords)
{
    return dense_bytes(count, maxRecords);   // (a multiple of 16)
}
constexpr uint64_t streams_bytes(uint64_t count, uint64_t maxRecords)
{
    return streams_next_offset(count, maxRecords) + ((count * 4 + 15) & ~(uint64_t)15);
}
constexpr uint64_t streams_scratch_offset(uint64_t count, uint64_t maxRecords)
{
    return streams_bytes(count, maxRecords);
}
constexpr uint64_t streams_stage_bytes(uint64_t count, uint64_t maxFrames, uint64_t maxRecords)
{
    return streams_scratch_offset(count, maxRecords) + count * maxFrames * sizeof(PackedHead);
}

/// Duplex byte-stream rows (k_ackstreamwalk, k_rowsum2, k_compact and k_slots,
/// sgpu_frames_scan_duplex_streams): the stream rows above with acknowledgement
/// frames accepted.  The output is the duplex dense layout (duplex_dense_bytes)
/// and behind it
///   count next words | zeros to the next 16-byte boundary
/// where row word k is k_ackwalk's and may also carry kStreamPartialDuplex, and
/// next_k is stream_walk's (frames.h ack_stream_walk states the walk).  The
/// partial flag has a bit of its own here: kStreamPartial is kPackedAcksDropped's
/// bit, and a duplex stream row can have dropped an ack and stop at a partial
/// frame in one scan.
///
/// On the device the walk takes one lane per row, kAckStreamWalkThreads rows per
/// workgroup (k_ackwalkd's scheme: DESIGN.md 2.2 has the measurement that ruled
/// out a second wave-per-row walk); its scratch areas lie behind the output in
/// the duplex dense scan's order.  Every offset below is a multiple of 16.
constexpr uint32_t kStreamPartialDuplex = 0x10000000u;
constexpr uint32_t kAckStreamWalkThreads = 256;
constexpr uint64_t duplex_streams_next_offset(uint64_t count, uint64_t maxRecords, uint64_t maxAcks,
                                              uint64_t ackBytes)
{
    return duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes);
}
constexpr uint64_t duplex_streams_bytes(uint64_t count, uint64_t maxRecords, uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_streams_next_offset(count, maxRecords, maxAcks, ackBytes) + ((count * 4 + 15) & ~(uint64_t)15);
}
constexpr uint64_t duplex_streams_scratch_records(uint64_t count, uint64_t maxRecords, uint64_t maxAcks,
                                                  uint64_t ackBytes)
{
    return duplex_streams_bytes(count, maxRecords, maxAcks, ackBytes);
}
constexpr uint64_t duplex_streams_scratch_slots(uint64_t count, uint64_t maxFrames, uint64_t maxRecords,
                                                uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_streams_scratch_records(count, maxRecords, maxAcks, ackBytes) +
           count * maxFrames * sizeof(PackedHead);
}
constexpr uint64_t duplex_streams_scratch_counts(uint64_t count, uint64_t maxFrames, uint64_t ackSlots,
                                                 uint64_t maxRecords, uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_streams_scratch_slots(count, maxFrames, maxRecords, maxAcks, ackBytes) +
           count * ackSlots * ackBytes;
}
constexpr uint64_t duplex_streams_stage_bytes(uint64_t count, uint64_t maxFrames, uint64_t ackSlots,
                                              uint64_t maxRecords, uint64_t maxAcks, uint64_t ackBytes)
{
    return duplex_streams_scratch_counts(count, maxFrames, ackSlots, maxRecords, maxAcks, ackBytes) +
           ((count * 4 + 15) & ~(uint64_t)15);
}

constexpr unsigned kTileBytes = 1024;       // solve tiles: 64 lanes x 16 bytes
constexpr unsigned kIngestChunkBytes = 8192;   // k_ingest: bytes per wave (8 x 1 KiB tiles)
/// Solves with more rows than this stage 256-byte tiles (16 lanes x 16 bytes
/// per row, four rows per wave) so all m <= 255 rows and the m x m
/// coefficients still fit one workgroup's LDS.
constexpr unsigned kSolveWideMaxRows = 120;
constexpr unsigned kSolveNarrowTileBytes = 256;
inline unsigned solve_tile_bytes(uint32_t m)
{
    return m > kSolveWideMaxRows ? kSolveNarrowTileBytes : kTileBytes;
}
/// Recovery-matrix generation + Gaussian elimination of one decode on the
/// device (k_ge; reference SiameseDecoder.cpp:2157-2531, the host's
/// generate_matrix + gaussian_elimination).  A job is a FRESH matrix of
/// `rows` recovery rows x `cols` lost columns (rows >= cols):
///   input (16-byte aligned, at GeDesc.in in the upload):
///     GeRow[rows], GeCol[cols], then pickLen bytes of pick columns: the
///     matrix column of window element pickLo + x (0xff: received);
///   output (GeDesc.result words of the result array, ge_result_words):
///     [0] the first pivot whose column has no non-zero left (== cols: the
///         matrix was eliminated), [1..2] the elimination's multiplied bytes
///         (the reference's muladds, u64), [3] 1 when [0] == cols, else 0,
///     [4] the non-zero coefficients below the diagonal of the eliminated
///         matrix in pivot order (MultiplyLowerTriangle's muladds per row
///         byte), [5..7] 0;
///     then the pivots (u8 row index per pivot position, padded to words);
///     without kGeChained also the used rows (u8 0/1), the column counts
///     (u16) and the matrix, rows x cols bytes in row order.
/// kGeChained (rows == cols): the decode's elimination of received data and
/// its solve were queued in the same submission, gated on word [3] (OP_ROWS
/// GfOp.termBegin, SolveDesc.gate).  On success the job writes the solve's
/// coefficients in pivot order (coef + solveCoef, cols x cols) and permutes
/// the solve's rows (rows + solveRow) into pivot order, each keeping its head
/// slot (SolveRow.headIndex).
/// A chained job whose solve the host could not queue (Program::solve_commit
/// never matched it) owns none: assembly replaces it by a 1 x 1 job of one
/// parity row without columns (a zero matrix), which reports outcome [3] = 0
/// and touches no solve, so every item gated on it is skipped.
/// Row kinds: Siamese (dense over [0, jEnd) from the row's opcodes, then
/// 2*ceil(ldpcN/16) PCG picks over [pickOff, pickOff + ldpcN)), Cauchy
/// (1/((rbase) ^ ccol) over [0, jEnd)) and parity (1 over [0, jEnd)).
struct GeDesc
{
    uint32_t in;        // byte offset of the job's input in the upload
    uint32_t result;    // first result word
    uint16_t rows, cols;
    uint32_t pickLen;
    uint32_t flags;     // kGeChained
    uint32_t solveRow;  // kGeChained: the solve's first SolveRow
    uint32_t solveCoef; // kGeChained: its coefficients' byte offset
    uint32_t pad;
};
static_assert(sizeof(GeDesc) == 32, "GeDesc layout");
constexpr uint32_t kGeChained = 1;

enum : uint8_t
{
    GE_SIAMESE = 0,
    GE_CAUCHY = 1,
    GE_PARITY = 2
};

struct GeRow
{
    uint16_t row;        // Siamese row number (opcodes, RX) / unused
    uint8_t kind;        // GE_*
    uint8_t rbase;       // Cauchy: (uint8)(row - 1 + kCauchyMaxColumns)
    uint16_t jEnd;       // dense columns [0, jEnd)
    uint16_t colCount;   // the row's column count (RecoveryPacket lost count)
    uint32_t ldpcN;      // Siamese: picks draw over ldpcN window elements
    uint32_t pickOff;    // ... starting at this index of the pick table
};

struct GeCol
{
    uint8_t lane;        // column % kLanes
    uint8_t cx, cx2;     // CX(column), CX(column)^2
    uint8_t ccol;        // column % kCauchyMaxColumns
};

/// Device elimination limits (LDS-resident matrix of one wave): the
/// reference's 255 lost columns (SiameseCommon.h:80, kMaximumLossRecoveryCount)
/// and up to 256 recovery rows.
constexpr unsigned kGeMaxCols = 255;
constexpr unsigned kGeMaxRows = 256;
constexpr unsigned kGeMaxPick = 65535;
constexpr uint8_t kGeNoColumn = 0xff;
/// k_ge's LDS row stride in dwords: odd, so the rows a wave's lanes own
/// start in different banks.
constexpr uint32_t ge_stride_words(uint32_t cols) { return ((cols + 3u) / 4u) | 1u; }

constexpr uint32_t ge_input_bytes(uint32_t rows, uint32_t cols, uint32_t pickLen)
{
    return (rows * 16u + cols * 4u + pickLen + 15u) & ~15u;
}
/// Word offsets of the output parts (ge_result_words: the total).
constexpr uint32_t kGeOutHeader = 8;
constexpr uint32_t ge_out_pivots(uint32_t) { return kGeOutHeader; }
constexpr uint32_t ge_out_used(uint32_t rows) { return kGeOutHeader + (rows + 3) / 4; }
constexpr uint32_t ge_out_counts(uint32_t rows) { return kGeOutHeader + 2 * ((rows + 3) / 4); }
constexpr uint32_t ge_out_matrix(uint32_t rows) { return ge_out_counts(rows) + (rows + 1) / 2; }
constexpr uint32_t ge_result_words(uint32_t rows, uint32_t cols, bool chained = false)
{
    return chained ? ge_out_used(rows) : ge_out_matrix(rows) + (rows * cols + 3) / 4;
}

constexpr uint32_t kNoRows = 0xffffffffu;   // be_launch_exec: no OP_ROWS in the launch
constexpr unsigned kExecTileBytes = 256;    // executor tiles: 64 lanes x 4 bytes

} // namespace sgpu
