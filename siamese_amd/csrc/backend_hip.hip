// backend_hip.hip -- gfx950 kernels and the HIP side of backend.h.
//
// Kernels (all byte-column local, see ops.h):
//   k_ingest       copy symbols (with their length prefix) into fresh buffers,
//                  8 KiB chunks of a symbol dealt to separate waves
//   k_exec         run one segment of every instance's op list on one
//                  256-byte tile (64 lanes x 4 bytes; 16 waves share the
//                  tile's terms): LINCOMB = XOR / GF(256) multiply-accumulate
//                  of up to thousands of source symbols into one destination,
//                  OP_ROWS Siamese row batches staged in LDS
//   k_ldpc         the LDPC picks of wide rows (windows of >= 512 elements)
//   k_solve_pre    per solve: bytes 0..3 of every row (the recovered lengths,
//                  one wave) beside the inverse T = U^-1 L^-1 of its matrix
//   k_solve_tr     X = T R on the vector ALUs, per (solve, 1 KiB tile)
//   k_solve_main   the copy of a product-solved tile, or lower-triangle
//                  multiply + back-substitution per tile (the reference's
//                  sweeps: small launches, flagged solves)
//   k_solve_prefix the length pass alone (sweeps-only launches)
//   k_ge           a decode's recovery matrix and its elimination (opt-in)
//   k_deliver      decoded packets into caller-owned rows at a fixed stride,
//                  lengths beside them (k_ingest backwards, opt-in)
//   k_relay        a decoder's packets forwarded as originals' wire frames, the
//                  header computed from the length read on the device
//   k_plan, k_pack the same frames several to a row: the packer's layout made
//                  on the device from those lengths, then k_relay's copy
//   k_offsets, k_concat  decoded packets as one contiguous byte stream: a prefix
//                  sum over those lengths, then a copy to byte-granular offsets
//   k_frame        a sender's originals and recovery packets as wire frames
//                  into caller-owned rows (header, packet, zero tail; opt-in)
//   k_scan         frame rows in device memory into 32-byte host records
//   k_walk         rows that hold several frames into one record per frame
//   k_walkd, k_rowsum, k_compact  k_walk's records of all rows back to back: the
//                  walk into device scratch, a prefix sum over the rows' counts,
//                  then a placed copy
//   k_ackwalk      k_walk with acknowledgement frames, their messages into slots
//   k_ackwalkd, k_rowsum2, k_slots  k_ackwalk's records (through k_compact) and
//                  used slots of all rows back to back: the walk into device
//                  scratch, one prefix sum over both counts, then placed copies
//   k_ackstreamwalk  k_ackwalkd for rows that are byte streams: bytes [start,
//                  end), a cut-off last frame reported as partial, a next word
//                  (header fields, a recovery packet's head and tail; opt-in)
//
// GF(256) multiply by a wave-uniform constant uses three v_perm_b32 byte
// lookups per dword (bits 0-2, 3-5, 6-7 of each byte) and one v_bitop3_b32
// to XOR them; the 32-byte table per constant lives in constant memory.  The
// algorithmic roofline is HBM bandwidth, but the measured bounds are
// on-chip: k_exec waits on LDS staging and its per-op barriers (SQ_WAIT_ANY
// ~60 %, real HBM traffic about a tenth of peak), k_solve_tr on v_perm_b32
// issue (half rate) and its per-pivot waits.
#include <hip/hip_runtime.h>

#include "backend.h"
#include "codedef.h"
#include "placement.h"
#include "pool.h"
#include "gf.h"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <type_traits>
#include <cstring>
#include <ctime>
#include <deque>
#include <mutex>
#include <vector>

namespace sgpu {

// ---------------------------------------------------------------------------
// Device tables

// device (global) address space: plain global_load/store rather than flat
// ones, which would also count against lgkmcnt and make every LDS wait wait
// for outstanding memory loads
#define GMEM __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__constant__ uint32_t c_perm[256][8];   // per constant y: {Ta0,Ta1,Tb0,Tb1,Tc,0,0,0}
__constant__ __attribute__((aligned(16))) uint8_t c_inv[256];   // (read as dwords too)

// The inverse of a wave-uniform y through the scalar data cache: c_inv[y]
// compiles to a vector memory load (a full memory round trip on a solve's
// serial pivot chain); the dword holding it, uniformly indexed, is a scalar
// load.
__device__ __forceinline__ uint32_t inv_u(uint32_t y)
{
    const uint32_t w = reinterpret_cast<const uint32_t*>(c_inv)[__builtin_amdgcn_readfirstlane(y) >> 2];
    return (w >> (8u * (y & 3u))) & 0xffu;
}

__device__ __forceinline__ uint32_t gf_mul_dword(uint32_t x, uint32_t y)
{
    const uint32_t* t = c_perm[y];
    const uint32_t a = x & 0x07070707u;
    const uint32_t b = (x >> 3) & 0x07070707u;
    const uint32_t c = (x >> 6) & 0x03030303u;
    // (v_bitop3_b32 0x96: the three lookups' XOR in one full-rate instruction)
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(t[1], t[0], a), __builtin_amdgcn_perm(t[3], t[2], b),
                                       __builtin_amdgcn_perm(0u, t[4], c), 0x96);
}

// the same multiply with y's three lookup words already in registers (per
// lane, or moved to scalars with readlane), so no table fetch sits in a loop
struct GfTab
{
    uint32_t a0, a1, b0, b1, c;
};

__device__ __forceinline__ GfTab gf_tab(uint32_t y)
{
    const uint32_t* t = c_perm[y];
    return GfTab{t[0], t[1], t[2], t[3], t[4]};
}

// from the workgroup's LDS copy of c_perm (a0 a1 b0 b1 | c)
__device__ __forceinline__ GfTab gf_tab_l(const uint4* permL, const uint32_t* permC, uint32_t y)
{
    const uint4 t = permL[y];
    return GfTab{t.x, t.y, t.z, t.w, permC[y]};
}

__device__ __forceinline__ uint32_t gf_mul_tab(uint32_t x, const GfTab& t)
{
    const uint32_t a = x & 0x07070707u;
    const uint32_t b = (x >> 3) & 0x07070707u;
    const uint32_t c = (x >> 6) & 0x03030303u;
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(t.a1, t.a0, a), __builtin_amdgcn_perm(t.b1, t.b0, b),
                                       __builtin_amdgcn_perm(0u, t.c, c), 0x96);
}

__device__ __forceinline__ uint4 gf_mul16(uint4 v, uint32_t y)
{
    uint4 r;
    r.x = gf_mul_dword(v.x, y);
    r.y = gf_mul_dword(v.y, y);
    r.z = gf_mul_dword(v.z, y);
    r.w = gf_mul_dword(v.w, y);
    return r;
}

__device__ __forceinline__ uint4 gf_mul16_tab(uint4 v, const GfTab& t)
{
    return make_uint4(gf_mul_tab(v.x, t), gf_mul_tab(v.y, t), gf_mul_tab(v.z, t), gf_mul_tab(v.w, t));
}

// A source row's 16 bytes split into the three bit groups gf_mul_tab looks
// up, once per pivot step instead of once per row update
// (k_solve_main 295 -> 270 us per C4 launch; profiles/r3k_solve_ab.txt)
struct Split16
{
    uint32_t a[4], b[4], c[4];
};

__device__ __forceinline__ Split16 gf_split16(uint4 v)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    Split16 s;
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        s.a[k] = w[k] & 0x07070707u;
        s.b[k] = (w[k] >> 3) & 0x07070707u;
        s.c[k] = (w[k] >> 6) & 0x03030303u;
    }
    return s;
}

__device__ __forceinline__ uint4 gf_mul16_split(const Split16& s, const GfTab& t)
{
    uint32_t r[4];
#pragma unroll
    for (unsigned k = 0; k < 4; ++k)
        r[k] = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(t.a1, t.a0, s.a[k]),
                                           __builtin_amdgcn_perm(t.b1, t.b0, s.b[k]),
                                           __builtin_amdgcn_perm(0u, t.c, s.c[k]), 0x96);
    return make_uint4(r[0], r[1], r[2], r[3]);
}

__device__ __forceinline__ uint32_t byte_mask(int n)
{
    // mask of the low n bytes of a dword, n clamped to [0,4]
    return n <= 0 ? 0u : (n >= 4 ? 0xffffffffu : ((1u << (8 * n)) - 1u));
}

__device__ __forceinline__ uint4 mask16(uint4 v, int nbytes)
{
    v.x &= byte_mask(nbytes);
    v.y &= byte_mask(nbytes - 4);
    v.z &= byte_mask(nbytes - 8);
    v.w &= byte_mask(nbytes - 12);
    return v;
}

__device__ __forceinline__ uint4 xor16(uint4 a, uint4 b)
{
    return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}

// a ^ b ^ c ^ d ^ e: two full-rate v_bitop3_b32 (0x96, three-way XOR) per
// dword instead of four XORs
__device__ __forceinline__ uint32_t xor5(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e)
{
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(a, b, c, 0x96), d, e, 0x96);
}
__device__ __forceinline__ uint4 xor5_16(uint4 a, uint4 b, uint4 c, uint4 d, uint4 e)
{
    return make_uint4(xor5(a.x, b.x, c.x, d.x, e.x), xor5(a.y, b.y, c.y, d.y, e.y), xor5(a.z, b.z, c.z, d.z, e.z),
                      xor5(a.w, b.w, c.w, d.w, e.w));
}

__device__ __forceinline__ uint4 ld16(uint64_t addr)
{
    const u32x4 r = *reinterpret_cast<const GMEM u32x4*>(addr);
    return make_uint4(r.x, r.y, r.z, r.w);
}

__device__ __forceinline__ void st16(uint64_t addr, uint4 v)
{
    *reinterpret_cast<GMEM u32x4*>(addr) = u32x4{v.x, v.y, v.z, v.w};
}

// ---------------------------------------------------------------------------
// Ingest

// One wave per (symbol, 8 KiB chunk) -- blockIdx.y is the chunk, so a
// 64 KiB symbol is copied by nine waves across the chip instead of one wave
// looping over it; lane L of each 1 KiB tile writes dst bytes [16L, 16L+16).  The source is shifted by the 1-4 byte length prefix, so a
// lane's 16 bytes straddle two aligned 16-byte source words: both are loaded
// (coalesced) and recombined with v_alignbyte_b32.  The word offset and byte
// shift are uniform per symbol, so the selection is a uniform branch, not a
// register-indexed gather.  Every lane takes the same path: only aligned
// words holding at least one source byte are loaded (an aligned 16-byte word
// never crosses a page), the prefix bytes are merged into lane 0 and bytes
// past the symbol are masked to zero.  Two tiles' loads are in flight before
// their stores.
//
// Runs (IngestDesc.count > 1): with a block table, workgroup b takes table
// entry blocks[b] = descriptor << 4 | group, and wave w copies symbol
// 4 * group + w of that run; without one (the gather path), wave w of
// workgroup b copies descriptor 4 b + w, a run of one.

__device__ __forceinline__ uint32_t pick(const uint32_t* w, unsigned q, unsigned r, unsigned k)
{
    return __builtin_amdgcn_alignbyte(w[q + k + 1], w[q + k], r);
}

__global__ __launch_bounds__(64 * kIngestWaves) void k_ingest(const IngestDesc* __restrict__ descs,
                                                              uint32_t count, const uint32_t* __restrict__ blocks)
{
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t di, k;
    if (blocks) {
        const uint32_t e = blocks[blockIdx.x];
        di = e >> 4;
        k = (e & 15u) * kIngestWaves + wave;
    } else {
        di = blockIdx.x * kIngestWaves + wave;
        k = 0;
    }
    if (di >= count)
        return;
    const uint32_t lane = threadIdx.x & 63;
    IngestDesc d = descs[di];
    if (k >= (d.count ? d.count : 1u))
        return;
    d.dst2 = (d.dst2Mask >> k & 1u) ? d.dst2 + (uint64_t)k * d.dstStride : 0;
    if (k) {
        d.src += (uint64_t)k * d.srcStride;
        d.dst += (uint64_t)k * d.dstStride;
    }
    const uint32_t total = d.hdrLen + d.bytes;
    // source address that lines up with dst byte 0
    const uint64_t base = d.src - d.hdrLen;
    const unsigned sh = (unsigned)(base & 15u);
    const unsigned q = sh >> 2, r = sh & 3;
    const uint64_t srcEnd = d.src + d.bytes;
    const uint32_t h0 = d.hdr[0] | (d.hdr[1] << 8) | (d.hdr[2] << 16) | ((uint32_t)d.hdr[3] << 24);
    const uint32_t h1 = d.hdr[4] | (d.hdr[5] << 8) | (d.hdr[6] << 16) | ((uint32_t)d.hdr[7] << 24);
    const uint32_t c0 = blockIdx.y * kIngestChunkBytes;
    const uint32_t c1 = c0 + kIngestChunkBytes < total ? c0 + kIngestChunkBytes : total;

    for (uint32_t t = c0; t < c1; t += 2 * kTileBytes) {
        uint4 out[2];
#pragma unroll
        for (unsigned u = 0; u < 2; ++u) {
            const uint32_t p = t + u * kTileBytes + lane * 16;
            out[u] = make_uint4(0, 0, 0, 0);
            if (p >= total)
                continue;
            const uint64_t a = (base + p) & ~(uint64_t)15;
            const bool any = d.bytes != 0;
            const uint4 lo = (any && a < srcEnd && a + 16 > d.src) ? ld16(a) : make_uint4(0, 0, 0, 0);
            const uint4 hi = (any && sh != 0 && a + 16 < srcEnd) ? ld16(a + 16) : make_uint4(0, 0, 0, 0);
            const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            switch (q) {   // wave-uniform
            case 0:
                out[u] = make_uint4(pick(w, 0, r, 0), pick(w, 0, r, 1), pick(w, 0, r, 2), pick(w, 0, r, 3));
                break;
            case 1:
                out[u] = make_uint4(pick(w, 1, r, 0), pick(w, 1, r, 1), pick(w, 1, r, 2), pick(w, 1, r, 3));
                break;
            case 2:
                out[u] = make_uint4(pick(w, 2, r, 0), pick(w, 2, r, 1), pick(w, 2, r, 2), pick(w, 2, r, 3));
                break;
            default:
                out[u] = make_uint4(pick(w, 3, r, 0), pick(w, 3, r, 1), pick(w, 3, r, 2), pick(w, 3, r, 3));
                break;
            }
        }
#pragma unroll
        for (unsigned u = 0; u < 2; ++u) {
            const uint32_t p = t + u * kTileBytes + lane * 16;
            if (p >= total)
                continue;
            uint4 v = out[u];
            if (p == 0) {   // the length prefix (at most 8 bytes) over source bytes
                const uint32_t m0 = byte_mask((int)d.hdrLen), m1 = byte_mask((int)d.hdrLen - 4);
                v.x = (v.x & ~m0) | (h0 & m0);
                v.y = (v.y & ~m1) | (h1 & m1);
            }
            if (p + 16 > total)
                v = mask16(v, (int)total - (int)p);
            st16(d.dst + p, v);
            if (d.dst2)   // (uniform)
                st16(d.dst2 + p, v);
        }
    }
}

// ---------------------------------------------------------------------------
// Executor
//
// One workgroup of kExecWaves waves per (instance segment, 256-byte tile):
// lane L owns bytes [4L, 4L+4) of the tile, so a 1402-byte symbol spans six
// work items and a 64 KiB symbol 256, and every source costs a wave one
// 256-byte coalesced load (global_load_dword) or LDS read.
//
// The segment is one instruction stream (ops.h): each op's header and its
// words are contiguous, and the workgroup keeps the current op's first
// kRingWords words in an LDS ring while one coalesced load per thread
// prefetches the next op's, so no op waits on a descriptor round trip.
//
//   OP_LINCOMB  terms dealt to the waves in contiguous shares (kExecDepth
//               loads in flight per wave), partial sums meet in LDS, wave 0
//               merges and stores.
//   OP_ROWS     the batch's window snapshot is staged in LDS: the tile's 256
//               bytes of up to `stage` window symbols (one coalesced
//               bulk load), so every later read of a symbol by the batch's
//               sum updates and rows is an LDS read instead of an HBM/L2
//               round trip.  The lane-sum updates are dealt to the waves
//               whole (each wave generates its element terms and CX
//               coefficients), one barrier, then the rows: with at least as
//               many rows as waves each wave takes whole rows; with fewer,
//               each row's LDPC picks are split across W/R waves (PCG
//               jump-ahead to each part's first draw) and the partial sums
//               meet in LDS, so a single large row (C3/C5) still keeps every
//               wave busy.
//   OP_COPIES   independent copies dealt to the waves, four at a time.
// The barrier that rotates the ring also orders each op's stores before any
// later op of the segment reads them (stores from one CU are visible to the
// CU's other waves after the workgroup-scope fence of __syncthreads).
#ifndef SGPU_EXEC_WAVES
#define SGPU_EXEC_WAVES 16
#endif
constexpr unsigned kExecWaves = SGPU_EXEC_WAVES;
constexpr unsigned kExecThreads = 64 * kExecWaves;
constexpr unsigned kExecDepth = 16;          // term loads in flight per wave
constexpr unsigned kExecSolo = 4;            // ops with <= this many terms run on wave 0 alone
constexpr unsigned kRingWords = 256;         // prefetched words per op (threads < 256 fetch one)
#ifndef SGPU_STAGE_PRE
#define SGPU_STAGE_PRE 2
#endif
constexpr unsigned kStagePre = SGPU_STAGE_PRE;   // stage entries per thread fetched a tile ahead (<= 4: VGPRs)
// (kRowsTableLds, the sum + window descriptors of an OP_ROWS batch in LDS: ops.h)
constexpr unsigned kPlanCap = 8192;          // planned row terms (LDS slot indices) per batch
constexpr unsigned kPlanRows = 256;          // rows of a batch that get a plan
constexpr uint32_t kNoPlan = 0xffffffffu;    // row not planned: general path, counts its bytes
constexpr uint32_t kPlanGeneral = 0xfffffffeu;   // planned and counted, but reads memory
static_assert(kExecTileBytes == 256, "executor tile = 64 lanes x 4 bytes");

__constant__ uint64_t c_pcgA[65];   // A^j
__constant__ uint64_t c_pcgG[65];   // sum_{t<j} A^t
__constant__ uint64_t c_pcgJA[32];  // A^(2^k)
__constant__ uint64_t c_pcgJG[32];  // sum_{t<2^k} A^t
__constant__ uint8_t c_sqr[256];

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// v, as a value the compiler cannot prove loop invariant (so loads indexed by
// it are not hoisted out of the loop and kept live in registers)
__device__ __forceinline__ uint32_t opaque(uint32_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// add a per-lane count to the workgroup's LDS counter: one atomic per wave
// (a global atomic per lane serialises at one L2 address across the grid)
__device__ __forceinline__ void acct_wave(unsigned long long* acctL, uint32_t v)
{
#pragma unroll
    for (unsigned d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(acctL, (unsigned long long)v);
}

#ifdef SGPU_PHASE_CLOCKS
// profiling build only: shader clocks per OP_ROWS phase, summed over
// workgroups as seen by thread 0 (tools/phase_clocks.py reads them)
__device__ unsigned long long g_phaseClk[64];
#define PHASE_MARK(k, t)                                                             \
    do {                                                                             \
        if (tid == 0) {                                                              \
            const unsigned long long now_ = clock64();                               \
            atomicAdd(&g_phaseClk[k], now_ - (t));                                   \
            (t) = now_;                                                              \
        }                                                                            \
    } while (0)
#define PHASE_ADD(k, v)                                                              \
    do {                                                                             \
        if ((threadIdx.x & 63) == 0)                                                 \
            atomicAdd(&g_phaseClk[k], (unsigned long long)(v));                      \
    } while (0)
#define PHASE_CLK() clock64()
#else
#define PHASE_MARK(k, t) (void)0
#define PHASE_ADD(k, v) (void)0
#define PHASE_CLK() 0ull
#endif

__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t lane)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

__device__ __forceinline__ uint32_t ld4(uint64_t addr)
{
    return *reinterpret_cast<const GMEM uint32_t*>(addr);
}

__device__ __forceinline__ void st4(uint64_t addr, uint32_t v)
{
    *reinterpret_cast<GMEM uint32_t*>(addr) = v;
}

// A term's bytes in [len, align16(len)) are zero in memory (every writer
// zero-fills the tail of its last 16-byte lane, ops.h), so only lanes wholly
// past the term's end need clearing.
__device__ __forceinline__ uint32_t term_load(uint64_t src, uint32_t len, uint32_t p)
{
    return p < len ? ld4(src + p) : 0u;
}

__device__ __forceinline__ uint32_t term_mul(uint32_t x, uint32_t coeff)
{
    return coeff == 1 ? x : gf_mul_dword(x, coeff);
}

// Word `idx` of the current op's block: from the LDS ring while it lasts,
// then straight from the stream.
__device__ __forceinline__ uint4 op_word(const uint4* ring, const uint4* __restrict__ seg, uint32_t pos,
                                         uint32_t idx)
{
    return idx < kRingWords ? ring[idx] : ld16((uint64_t)(seg + pos + idx));
}

// Accumulate terms [k0, k1).  fetch(k, src, len, ca) is called once per term
// with increasing k and describes term k (ca = coeff | acc << 8); it returns
// false for an absent term.  The loads of up to kExecDepth terms go out back
// to back before the first is used; a term that ends before the tile is not
// loaded.
template <bool Exact = false, class Fetch>
__device__ __forceinline__ void gather(uint32_t k0, uint32_t k1, uint32_t tileBase, uint32_t p,
                                       uint32_t& acc0, uint32_t& acc1, Fetch&& fetch)
// (Exact: bytes at or past a term's length read as zero even inside its last
// dword -- the lane sums of a row batch, which an update in the same batch may
// have grown past the length the row reads)
{
    for (uint32_t k = k0; k < k1; k += kExecDepth) {
        uint32_t v[kExecDepth], ca[kExecDepth];
        bool act[kExecDepth];
#pragma unroll
        for (unsigned u = 0; u < kExecDepth; ++u) {
            const uint32_t idx = k + u;
            uint64_t src = 0;
            uint32_t len = 0;
            act[u] = idx < k1 && fetch(idx, src, len, ca[u]) && tileBase < len;
            v[u] = act[u] ? term_load(src, len, p) : 0u;
            if (Exact && p < len)
                v[u] &= byte_mask((int)len - (int)p);
        }
#pragma unroll
        for (unsigned u = 0; u < kExecDepth; ++u) {
            if (act[u]) {
                const uint32_t x = term_mul(v[u], ca[u] & 0xff);
                if (ca[u] & 0xff00)
                    acc1 ^= x;
                else
                    acc0 ^= x;
            }
        }
    }
}

// term descriptor word held by lane j -> scalars
__device__ __forceinline__ void lane_term(uint4 w, uint32_t j, uint64_t& src, uint32_t& len)
{
    src = ((uint64_t)rl(w.y, j) << 32) | rl(w.x, j);
    len = rl(w.z, j);
}

__device__ __forceinline__ uint32_t align16u(uint32_t v) { return (v + 15u) & ~15u; }

// dst[p, p+4) of an item: keep(dst, valid) ^ out for bytes < n, zero for
// bytes in [n, align16(n)) (the zero tail every term reader relies on),
// nothing stored past that.  `cur` is dst[p, p+4) as loaded at item start.
__device__ __forceinline__ void store_item(uint32_t out, uint32_t p, uint64_t dst, uint32_t n, uint32_t valid,
                                           uint32_t cur)
{
    if (p >= align16u(n))
        return;
    if (p >= n) {
        st4(dst + p, 0u);
        return;
    }
    if (p < valid)
        out ^= cur & byte_mask((int)valid - (int)p);
    st4(dst + p, out & byte_mask((int)n - (int)p));
}

// the dword store_item writes at p < align16(n) (keep(cur, valid) ^ out,
// zero past n)
__device__ __forceinline__ uint32_t item_value(uint32_t out, uint32_t p, uint32_t n, uint32_t valid, uint32_t cur)
{
    if (p < valid)
        out ^= cur & byte_mask((int)valid - (int)p);
    return out & byte_mask((int)n - (int)p);
}

// store_item for a 16-byte lane (the quad layout of planned rows: lane
// holds bytes [p, p+16) of the tile)
__device__ __forceinline__ void store_item16(uint4 out, uint32_t p, uint64_t dst, uint32_t n, uint32_t valid,
                                             uint4 cur)
{
    if (p >= align16u(n))
        return;
    if (p < valid)
        out = xor16(out, mask16(cur, (int)valid - (int)p));
    st16(dst + p, mask16(out, (int)n - (int)p));
}

__device__ __forceinline__ uint4 load_cur16(uint32_t p, uint64_t dst, uint32_t n, uint32_t valid)
{
    return (p < n && p < valid) ? ld16(dst + p) : make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ uint4 lds16(const uint32_t* base, uint32_t word)
{
    return *reinterpret_cast<const uint4*>(base + word);
}

__device__ __forceinline__ uint4 and16(uint4 v, uint32_t m)
{
    return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
}

// lane K of each 16-lane row (quad) to the whole row: DPP row_newbcast, a
// VALU move (no LDS round trip)
template <unsigned K>
__device__ __forceinline__ uint32_t row_bcast(uint32_t v)
{
    static_assert(K < 16, "row lane");
    // (row_newbcast fills every lane: no old value to materialise)
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x150 + K, 0xf, 0xf, true);
}

// the four quads (16-lane groups) of a wave hold partial sums of one tile:
// fold them so every quad holds the total
__device__ __forceinline__ uint4 quad_fold(uint4 v)
{
    v.x ^= __shfl_xor(v.x, 16, 64);
    v.y ^= __shfl_xor(v.y, 16, 64);
    v.z ^= __shfl_xor(v.z, 16, 64);
    v.w ^= __shfl_xor(v.w, 16, 64);
    v.x ^= __shfl_xor(v.x, 32, 64);
    v.y ^= __shfl_xor(v.y, 32, 64);
    v.z ^= __shfl_xor(v.z, 32, 64);
    v.w ^= __shfl_xor(v.w, 32, 64);
    return v;
}

// what store_item needs of dst, loaded while the terms stream in
__device__ __forceinline__ uint32_t load_cur(uint32_t p, uint64_t dst, uint32_t n, uint32_t valid)
{
    return (p < n && p < valid) ? ld4(dst + p) : 0u;
}

// `litLen` (<= 8) literal bytes at dst + n, written by the lanes owning them
// (the lane owns bytes [p, p + width) of the tile)
__device__ __forceinline__ void store_literal(uint32_t p, uint64_t dst, uint32_t n, uint32_t litLen,
                                              uint32_t lit0, uint32_t lit1, uint32_t width = 4)
{
    if (litLen && n + litLen > p && n < p + width) {
        GMEM uint8_t* d = reinterpret_cast<GMEM uint8_t*>(dst);
        for (uint32_t k = (n > p ? n : p); k < n + litLen && k < p + width; ++k)
            d[k] = (uint8_t)(((k - n) >= 4 ? lit1 : lit0) >> (8 * ((k - n) & 3)));
    }
}

__device__ __forceinline__ uint32_t pcg_output(uint64_t s)
{
    const uint32_t xs = (uint32_t)(((s >> 18) ^ s) >> 27);
    const uint32_t r = (uint32_t)(s >> 59);
    return (xs >> r) | (xs << ((32u - r) & 31u));
}

// PCG state after d more draws from state s (uniform): the draws compose as
// powers of one affine map, applied per set bit of d.
__device__ __forceinline__ uint64_t pcg_jump(uint64_t s, uint64_t inc, uint32_t d)
{
    for (uint32_t k = 0; d; ++k, d >>= 1)
        if (d & 1u)
            s = c_pcgJA[k] * s + inc * c_pcgJG[k];
    return s;
}

// Sum or window descriptor i of the current OP_ROWS batch (per lane)
// (LDS slot j holds block word j < kRowSums, else word j + skip: window
// entries below the batch's stageLo, which only k_ldpc reads, stay in memory)
// (LDS slot j holds block word j < kRowSums, else word j + skip: window
// entries below the batch's stageLo, which only k_ldpc reads, stay in memory.
// table_entry: a word past the window (updates, rows); win_entry: window
// element e; table_word: any word)
// Fit: the whole block from `skip` lies in the LDS table (OP_ROWS checks it
// once per batch), so no read has a memory fallback: a fallback's load would
// make every later use wait for all of the wave's outstanding memory loads
// (the waits merge at the join), the update units' and rows' among them.
// (The executor reads no window element below skip: Program::rows_close.)
template <bool Fit>
__device__ __forceinline__ uint4 table_entry(const uint4* tableL, const uint4* __restrict__ seg,
                                             uint32_t blockWord, uint32_t i, uint32_t skip)
{
    const uint32_t j = i - skip;
    if constexpr (Fit)
        return tableL[j];
    else
        return j < kRowsTableLds ? tableL[j] : ld16((uint64_t)(seg + blockWord + i));
}
template <bool Fit>
__device__ __forceinline__ uint4 win_entry(const uint4* tableL, const uint4* __restrict__ seg, uint32_t blockWord,
                                           uint32_t e, uint32_t skip)
{
    const uint32_t j = e - skip;   // (wraps for e < skip)
    if constexpr (Fit)
        return tableL[kRowSums + j];
    else
        return j < kRowsTableLds - kRowSums ? tableL[kRowSums + j]
                                            : ld16((uint64_t)(seg + blockWord + kRowSums + e));
}
template <bool Fit>
__device__ __forceinline__ uint4 table_word(const uint4* tableL, const uint4* __restrict__ seg, uint32_t blockWord,
                                            uint32_t i, uint32_t skip)
{
    return i < kRowSums ? tableL[i] : win_entry<Fit>(tableL, seg, blockWord, i - kRowSums, skip);
}

// One Siamese row's LDPC picks [d0, d1) of PCG.Seed(row, N) (pair index
// d / 2; even draws feed acc0, odd acc1), from the staged window where it
// holds the element and from memory otherwise.  Returns the reference source
// bytes of the picks (SiameseEncoder.cpp:1100-1144 adds min(len, rowBytes)).
template <bool Fit>
__device__ __forceinline__ uint32_t row_picks(uint32_t row, uint32_t N, uint32_t off, uint32_t d0,
                                              uint32_t d1, uint32_t rn, uint32_t tileBase, uint32_t p,
                                              uint32_t lane, uint64_t pcgA, uint64_t pcgG,
                                              const uint32_t* stage, uint32_t stageLo, uint32_t staged,
                                              const uint4* tableL, const uint4* __restrict__ seg,
                                              uint32_t blk, uint32_t& acc0, uint32_t& acc1)
// (window element e in [stageLo, stageLo + staged) lives in stage slot
// kRowSums + e - stageLo)
{
    const uint64_t inc = ((uint64_t)row << 1) | 1u;
    uint64_t sc = pcg_jump((inc + N) * kPcgMul + inc, inc, d0);   // state after Seed(), then d0 draws
    uint32_t refBytes = 0;
    for (uint32_t c = d0; c < d1; c += 64) {
        // lane j: draw c + j -> window element e and its descriptor
        const uint64_t st = pcgA * sc + inc * pcgG;
        const uint32_t e = off + pcg_output(st) % N;
        const uint4 ev = win_entry<Fit>(tableL, seg, blk, e, stageLo);
        sc = c_pcgA[64] * sc + inc * c_pcgG[64];
        const uint32_t cnt = d1 - c < 64 ? d1 - c : 64;
        for (uint32_t j0 = 0; j0 < cnt; j0 += kExecDepth) {
            uint32_t v[kExecDepth];
#pragma unroll
            for (unsigned u = 0; u < kExecDepth; ++u) {
                const uint32_t j = j0 + u;
                v[u] = 0;
                if (j < cnt) {
                    const uint32_t ej = rl(e, j);
                    uint64_t src;
                    uint32_t len;
                    lane_term(ev, j, src, len);
                    refBytes += len < rn ? len : rn;
                    if (ej - stageLo < staged)
                        v[u] = stage[(kRowSums + ej - stageLo) * 64 + lane];
                    else if (tileBase < len)
                        v[u] = term_load(src, len, p);
                }
            }
#pragma unroll
            for (unsigned u = 0; u < kExecDepth; ++u) {
                if (((c + j0 + u) & 1u) == 0)
                    acc0 ^= v[u];
                else
                    acc1 ^= v[u];
            }
        }
    }
    return refBytes;
}

// k_ldpc: the LDPC picks of wide rows (ops.h LdpcItem), one workgroup of
// kLdpcWaves waves per item = (row, 1 KiB tile, kLdpcPairsPerItem pairs).
// Wave w takes a contiguous share of the item's draws: lane j generates draw
// c + j (PCG jump-ahead, as the executor does) and loads that element's
// descriptor, then the wave streams the elements' 16-byte lanes eight loads
// at a time, even draws into a0 and odd into a1 (SiameseEncoder.cpp:
// 1100-1144; the decoder's rows SiameseDecoder.cpp:996-1051 draw the same
// way).  The waves meet in LDS and the tile is XORed into the row's zeroed
// scratch pair with one atomic per dword: the items of one row are spread
// over the whole chip instead of running inside the codec's one workgroup
// per tile.
// Gated: the launch holds items of chained decodes (ops.h LdpcItem): the
// item's gate word comes from a parallel array by a wave-uniform (scalar)
// load, and an item whose outcome word is zero returns before it reads or
// writes anything else.  The ungated instantiation is the kernel as it was.
constexpr unsigned kLdpcWaves = 4;
#ifndef SGPU_LDPC_DEPTH
#define SGPU_LDPC_DEPTH 8
#endif
constexpr unsigned kLdpcDepth = SGPU_LDPC_DEPTH;   // loads in flight per lane

template <bool Gated>
__global__ __launch_bounds__(64 * kLdpcWaves) void k_ldpc(const LdpcItem* __restrict__ items,
                                                          unsigned long long* __restrict__ acct,
                                                          const uint32_t* __restrict__ gates,
                                                          const uint32_t* results)
{
    __shared__ uint4 part[kLdpcWaves][2][64];
    if (Gated) {
        // (block-uniform: every wave of the item leaves before the barrier)
        const uint32_t gate = gates[blockIdx.x];
        if (gate != 0 && results[gate - 1u] == 0u)
            return;
    }
    const LdpcItem it = items[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uni(threadIdx.x >> 6);
    const uint32_t p = it.tileBase + lane * 16u;
    const uint32_t pairs = it.pair1 - it.pair0;
    const uint32_t d0 = 2u * (it.pair0 + pairs * wave / kLdpcWaves);
    const uint32_t d1 = 2u * (it.pair0 + pairs * (wave + 1) / kLdpcWaves);
    const uint64_t inc = ((uint64_t)it.row << 1) | 1u;
    uint64_t sc = pcg_jump((inc + it.N) * kPcgMul + inc, inc, d0);   // after Seed(), then d0 draws
    const uint64_t pa = c_pcgA[lane], pg = c_pcgG[lane];
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    uint32_t refBytes = 0;
    for (uint32_t c = d0; c < d1; c += 64) {
        const uint64_t st = pa * sc + inc * pg;
        sc = c_pcgA[64] * sc + inc * c_pcgG[64];
        const uint32_t cnt = d1 - c < 64 ? d1 - c : 64;   // (uniform)
        const uint32_t e = it.off + pcg_output(st) % it.N;
        const uint4 ev = lane < cnt ? ld16(it.win + (uint64_t)e * 16u) : make_uint4(0, 0, 0, 0);
        refBytes += ev.z < it.n ? ev.z : it.n;
        for (uint32_t j0 = 0; j0 < cnt; j0 += kLdpcDepth) {
            uint4 v[kLdpcDepth];
#pragma unroll
            for (unsigned u = 0; u < kLdpcDepth; ++u) {
                const uint32_t j = j0 + u;
                v[u] = make_uint4(0, 0, 0, 0);
                if (j < cnt) {
                    const uint64_t src = ((uint64_t)rl(ev.y, j) << 32) | rl(ev.x, j);
                    const uint32_t len = rl(ev.z, j);
                    // (bytes in [len, align16(len)) are zero in memory)
                    if (p < len)
                        v[u] = ld16(src + p);
                }
            }
#pragma unroll
            for (unsigned u = 0; u < kLdpcDepth; u += 2) {
                a0 = xor16(a0, v[u]);       // (c and j0 are even: draw parity = u's)
                a1 = xor16(a1, v[u + 1]);
            }
        }
    }
    part[wave][0][lane] = a0;
    part[wave][1][lane] = a1;
    if (it.tileBase == 0) {
        // the reference's source bytes of these draws, once per row (tile 0)
        unsigned long long rb = refBytes;
#pragma unroll
        for (unsigned d = 32; d >= 1; d >>= 1)
            rb += __shfl_xor(rb, d, 64);
        if (lane == 0 && rb)
            atomicAdd(acct, rb);
    }
    __syncthreads();
    if (wave == 0) {
        uint4 s0 = part[0][0][lane], s1 = part[0][1][lane];
#pragma unroll
        for (unsigned w = 1; w < kLdpcWaves; ++w) {
            s0 = xor16(s0, part[w][0][lane]);
            s1 = xor16(s1, part[w][1][lane]);
        }
        // (scratch tiles are whole: span is a multiple of the tile)
        uint32_t* l0 = reinterpret_cast<uint32_t*>(it.dst + p);
        uint32_t* l1 = reinterpret_cast<uint32_t*>(it.dst + it.span + p);
        if (s0.x) atomicXor(l0 + 0, s0.x);
        if (s0.y) atomicXor(l0 + 1, s0.y);
        if (s0.z) atomicXor(l0 + 2, s0.z);
        if (s0.w) atomicXor(l0 + 3, s0.w);
        if (s1.x) atomicXor(l1 + 0, s1.x);
        if (s1.y) atomicXor(l1 + 1, s1.y);
        if (s1.z) atomicXor(l1 + 2, s1.z);
        if (s1.w) atomicXor(l1 + 3, s1.w);
    }
}

// Versioned sum reads (RowItem.cutoff, ops.h): a row's selected sums as it
// read them = the batch's final sums with the contributions of each update's
// elements at or past the row's cutoff taken back out.  Quad layout (planned
// rows): the lane holds bytes [p16, p16 + 16) of its quad's row; m0 / m1 /
// cut are the quad's row's masks and cutoff (per lane), `live` whether the
// row reaches this tile.
template <bool Fit>
__device__ __forceinline__ uint4 version_elem16(uint32_t e, uint32_t p16, uint32_t b4, const uint32_t* stage,
                                                uint32_t stageLo, uint32_t staged, const uint4* tableL,
                                                const uint4* __restrict__ seg, uint32_t blk)
{
    if (e - stageLo < staged)
        return lds16(stage, (kRowSums + e - stageLo) * 64 + b4);
    const uint4 d = win_entry<Fit>(tableL, seg, blk, e, stageLo);
    const uint64_t src = ((uint64_t)d.y << 32) | d.x;
    return p16 < d.z ? ld16(src + p16) : make_uint4(0, 0, 0, 0);
}

//
// One Siamese lane l at a time: its three sums fold the same elements (one
// residue class mod 8), so an element's corrections for the sums the row
// selects combine into one coefficient per accumulator (1 ^ CX ^ CX^2 as the
// masks pick them): one load and at most two multiplies per element.  A sum
// whose length ends inside this 16-byte lane is taken per sum, with its
// exact clip.
template <bool Fit>
__device__ __forceinline__ void version_lane16(uint32_t l, uint32_t m0, uint32_t m1, uint32_t cut, bool live,
                                               uint32_t p16, uint32_t b4, const uint32_t* updOfL,
                                               const uint32_t* updFromL, const uint32_t* updToL,
                                               const uint32_t* cxL, const uint4* permL, const uint32_t* permC,
                                               const uint32_t* stage, uint32_t stageLo, uint32_t staged,
                                               const uint4* tableL, const uint4* __restrict__ seg, uint32_t blk,
                                               uint4& a0, uint4& a1)
{
    {
        uint32_t lo = 0xffffffffu, hi = 0, full = 0, part = 0;
        uint32_t f[kSums], t[kSums];
#pragma unroll
        for (uint32_t s = 0; s < kSums; ++s) {
            const uint32_t k = l * kSums + s;
            f[s] = t[s] = 0;
            if (updOfL[k] == 0xffu)
                continue;
            const bool sel = ((m0 | m1) >> k) & 1u;
            const uint32_t slen = tableL[k].z;
            if (!live || !sel || p16 >= slen)
                continue;
            f[s] = updFromL[k];
            t[s] = updToL[k];
            const uint32_t first = cut <= f[s] ? f[s] : f[s] + ((cut - f[s] + kLanes - 1) / kLanes) * kLanes;
            if (first >= t[s])
                continue;
            if (p16 + 16 > slen) {
                part |= 1u << s;
                continue;
            }
            full |= 1u << s;
            lo = min(lo, first);
            hi = max(hi, t[s]);
        }
        // (lo: a lane element, every range of the lane shares its residue)
        for (uint32_t e = lo; e < hi; e += kLanes) {
            PHASE_ADD(24, 1);
            uint32_t y0 = 0, y1 = 0, cx = 0;
            bool need = false;
#pragma unroll
            for (uint32_t s = 0; s < kSums; ++s)
                need |= (full >> s & 1u) && s != 0 && e >= f[s] && e < t[s];
            if (need) {
                const uint32_t col = win_entry<Fit>(tableL, seg, blk, e, stageLo).w;
                cx = cxL[col % kColumnValuePeriod];
            }
#pragma unroll
            for (uint32_t s = 0; s < kSums; ++s) {
                if (!(full >> s & 1u) || e < f[s] || e >= t[s])
                    continue;
                const uint32_t k = l * kSums + s;
                const uint32_t c = s == 0 ? 1u : s == 1 ? (cx & 0xffu) : (cx >> 8);
                if ((m0 >> k) & 1u)
                    y0 ^= c;
                if ((m1 >> k) & 1u)
                    y1 ^= c;
            }
            if (!(y0 | y1))
                continue;
            const uint4 v = version_elem16<Fit>(e, p16, b4, stage, stageLo, staged, tableL, seg, blk);
            if (y0)
                a0 = xor16(a0, y0 == 1 ? v : gf_mul16_tab(v, gf_tab_l(permL, permC, y0)));
            if (y1)
                a1 = xor16(a1, y1 == 1 ? v : gf_mul16_tab(v, gf_tab_l(permL, permC, y1)));
        }
        // sums ending inside this lane: per sum, clipped to their length
        for (; part; part &= part - 1) {
            const uint32_t s = (uint32_t)__builtin_ctz(part);
            const uint32_t k = l * kSums + s;
            const uint32_t slen = tableL[k].z;
            const bool in0 = (m0 >> k) & 1u, in1 = (m1 >> k) & 1u;
            for (uint32_t e = cut <= f[s] ? f[s] : f[s] + ((cut - f[s] + kLanes - 1) / kLanes) * kLanes; e < t[s];
                 e += kLanes) {
                PHASE_ADD(25, 1);
                uint4 v = version_elem16<Fit>(e, p16, b4, stage, stageLo, staged, tableL, seg, blk);
                if (s != 0) {
                    const uint32_t col = win_entry<Fit>(tableL, seg, blk, e, stageLo).w;
                    const uint32_t cx = cxL[col % kColumnValuePeriod];
                    v = gf_mul16_tab(v, gf_tab_l(permL, permC, s == 1 ? (cx & 0xffu) : (cx >> 8)));
                }
                v = mask16(v, (int)slen - (int)p16);
                if (in0)
                    a0 = xor16(a0, v);
                if (in1)
                    a1 = xor16(a1, v);
            }
        }
    }
}

template <bool Fit>
__device__ __forceinline__ void row_versions16(uint32_t m0, uint32_t m1, uint32_t cut, bool live, uint32_t p16,
                                               uint32_t b4, const uint32_t* updOfL, const uint32_t* updFromL,
                                               const uint32_t* updToL, const uint32_t* cxL, const uint4* permL,
                                               const uint32_t* permC, const uint32_t* stage, uint32_t stageLo,
                                               uint32_t staged, const uint4* tableL, const uint4* __restrict__ seg,
                                               uint32_t blk, uint4& a0, uint4& a1)
{
    for (uint32_t l = 0; l < kLanes; ++l)
        version_lane16<Fit>(l, m0, m1, cut, live, p16, b4, updOfL, updFromL, updToL, cxL, permL, permC, stage, stageLo,
                       staged, tableL, seg, blk, a0, a1);
}

// The same for a row in the dword layout (general path: one wave, the lane
// holds bytes [p, p + 4)); m0 / m1 / cut are wave-uniform.
template <bool Fit>
__device__ __forceinline__ void row_versions4(uint32_t m0, uint32_t m1, uint32_t cut, uint32_t tileBase, uint32_t p,
                                              uint32_t lane, const uint32_t* updOfL, const uint32_t* updFromL,
                                              const uint32_t* updToL, const uint32_t* cxL, const uint32_t* stage,
                                              uint32_t stageLo, uint32_t staged, const uint4* tableL,
                                              const uint4* __restrict__ seg, uint32_t blk, uint32_t& acc0,
                                              uint32_t& acc1)
{
    for (uint32_t k = 0; k < kRowSums; ++k) {
        const bool in0 = (m0 >> k) & 1u, in1 = (m1 >> k) & 1u;
        if ((!in0 && !in1) || uni(updOfL[k]) == 0xffu)
            continue;
        const uint32_t from = uni(updFromL[k]), to = uni(updToL[k]);
        const uint32_t sidx = k % kSums;
        const uint32_t slen = uni(tableL[k].z);   // the sum's length as the row reads it (clips the terms)
        if (tileBase >= slen)
            continue;
        const uint32_t clip = byte_mask((int)slen - (int)p);
        for (uint32_t e = cut <= from ? from : from + ((cut - from + kLanes - 1) / kLanes) * kLanes; e < to;
             e += kLanes) {
            uint32_t v;
            const uint4 d = win_entry<Fit>(tableL, seg, blk, e, stageLo);
            if (e - stageLo < staged) {
                v = stage[(kRowSums + e - stageLo) * 64 + lane];
            } else {
                const uint64_t src = ((uint64_t)uni(d.y) << 32) | uni(d.x);
                const uint32_t len = uni(d.z);
                v = tileBase < len ? term_load(src, len, p) : 0u;
            }
            if (sidx != 0) {
                const uint32_t cx = cxL[uni(d.w) % kColumnValuePeriod];
                v = gf_mul_dword(v, sidx == 1 ? (cx & 0xffu) : (cx >> 8));
            }
            v &= clip;
            if (in0)
                acc0 ^= v;
            if (in1)
                acc1 ^= v;
        }
    }
}

__global__ __launch_bounds__(kExecThreads) void k_exec(const uint4* __restrict__ stream,
                                                       const ExecItem* __restrict__ items,
                                                       unsigned long long* __restrict__ acct,
                                                       const uint32_t* __restrict__ results,
                                                       uint32_t stageSlots)
{
    __shared__ uint4 ring[2][kRingWords];
    __shared__ __attribute__((aligned(16))) uint32_t part[kExecWaves][2][64];
    __shared__ uint4 tableL[kRowsTableLds];
    __shared__ uint32_t cxL[kColumnValuePeriod];   // CX(c) | CX(c)^2 << 8 by c mod 253
    __shared__ uint16_t plan[kPlanCap];            // rows' terms as stage slots
    __shared__ uint2 rowInfo[kPlanRows];           // plan offset (or kNoPlan/kPlanGeneral), n0 | n1 << 16
    __shared__ unsigned long long acctL;          // reference source bytes counted by this workgroup
    __shared__ uint32_t generalRows;               // a row of this OP_ROWS batch has no plan
    __shared__ uint32_t sumsDirty;                 // a staged lane sum must be re-read after the updates
    // versioned sum reads (RowItem.cutoff): per sum k, the batch's update of
    // it (index, or 0xff) and that update's element range [from, to)
    __shared__ uint32_t updOfL[kRowSums];
    __shared__ uint32_t updFromL[kRowSums], updToL[kRowSums];
    __shared__ uint32_t updMaxLast1;   // 1 + the last element any update of the batch folds in (0: none)
    __shared__ uint32_t updSpanL;      // elements of the batch's longest update
    __shared__ uint32_t laneModeL;     // updates folded per window lane (see phase A)
    // the version corrections of the batch's first kVersionRows rows (this
    // tile, dword layout), computed per lane sum in phase A
    __shared__ uint32_t corrL[kVersionRows][2][64];
    __shared__ uint4 permL[256];                   // c_perm[y] words 0..3
    __shared__ uint32_t permC[256];                // c_perm[y] word 4
    // stage slot k < 24: lane sum k after the batch's updates; slot 24 + e:
    // window element e < stageCap; slot stageSlots: zeros ((stageSlots + 1)
    // x 64 dwords in all)
    extern __shared__ __attribute__((aligned(16))) uint32_t stage[];
    const uint32_t stageCap = stageSlots > kRowSums ? stageSlots - kRowSums : 0;
    const uint32_t zeroSlot = stageSlots;   // (one more slot, all zero, for masked reads)
    const ExecItem it = items[blockIdx.x];
    const uint4* seg = stream + it.streamBegin;
    const uint32_t words = it.streamWords;
    const uint32_t wave = uni(threadIdx.x >> 6);   // (uniform: keeps wave-derived loops scalar)
    // this workgroup's tiles [tile0, tile0 + nTiles * 256): every op runs
    // over each of them in turn, so an OP_ROWS batch loads its table and
    // draws its row plans once for all of them
    const uint32_t tile0 = exec_first_tile(it.tiles) * kExecTileBytes;
    const uint32_t nTiles = exec_tile_count(it.tiles);
#ifdef SGPU_PHASE_CLOCKS
    unsigned long long kclk = clock64();
#endif

    {
        const uint32_t tid = threadIdx.x;
        if (tid < kRingWords)
            ring[0][tid] = tid < words ? ld16((uint64_t)(seg + tid)) : make_uint4(0, 0, 0, 0);
        for (uint32_t c = tid; c < kColumnValuePeriod; c += kExecThreads) {
        const uint32_t cx = 3u + (c * 199u) % kColumnValuePeriod;   // SiameseCommon.h:89-93
            cxL[c] = cx | ((uint32_t)c_sqr[cx] << 8);
        }
        if (tid == 0)
            acctL = 0;
        if (stageSlots && tid < 64)
            stage[zeroSlot * 64 + tid] = 0;
        if (tid < 256) {
            permL[tid] = make_uint4(c_perm[tid][0], c_perm[tid][1], c_perm[tid][2], c_perm[tid][3]);
            permC[tid] = c_perm[tid][4];
        }
    }
    __syncthreads();
#ifdef SGPU_PHASE_CLOCKS
    if (threadIdx.x == 0)
        atomicAdd(&g_phaseClk[32], clock64() - kclk);
#endif
    uint32_t cur = 0, pos = 0;
    for (uint32_t oi = 0; oi < it.opCount; ++oi) {
#ifdef SGPU_PHASE_CLOCKS
        const unsigned long long oclk = clock64();
        unsigned long long t5 = 0;   // thread 0 past an OP_ROWS op's last phase
#endif
        // the thread index, opaque per op: lane-derived addresses are then
        // computed where they are used instead of hoisted out of the op loop,
        // where dozens of them would hold VGPRs through every phase
        const uint32_t tid = opaque(threadIdx.x);
        const uint32_t lane = tid & 63;
        const uint4* rb = ring[cur];
        const uint4 h0 = rb[0], h1 = rb[1];
        const uint64_t dst = ((uint64_t)uni(h0.y) << 32) | uni(h0.x);
        const uint32_t n = uni(h0.z), valid = uni(h0.w);
        const uint32_t kind = uni(h1.x);
        uint32_t itemWords = kOpWords;
        if (kind == OP_LINCOMB || kind == OP_ROWS || kind == OP_COPIES || kind == OP_LINCOMBS)
            itemWords += uni(h1.w);
        const uint32_t next = pos + itemWords;
        // prefetch the next op's block while this one runs
        uint4 pf = make_uint4(0, 0, 0, 0);
        if (tid < kRingWords && oi + 1 < it.opCount && next + tid < words)
            pf = ld16((uint64_t)(seg + next + tid));

        // an op gated on a chained device elimination that failed (GfOp
        // termBegin: 1 + its outcome word, ops.h) does nothing
        const uint32_t gate = kind != OP_LITERAL ? uni(h1.z) : 0u;
        const bool skip = gate != 0 && results[gate - 1u] == 0u;
        if (skip) {
        } else if (kind == OP_LITERAL) {
            if (wave == 0) {
                for (uint32_t ti = 0; ti < nTiles; ++ti)
                    store_literal(tile0 + ti * kExecTileBytes + lane * 4, dst, n, valid, uni(h1.z), uni(h1.w));
            }
        } else if (kind == OP_LINCOMB) {
            for (uint32_t ti = 0; ti < nTiles; ++ti) {
                // (lane-derived values re-derived per tile: hoisted out of the
                // tile loop they would hold VGPRs through every phase)
                const uint32_t tid = opaque(threadIdx.x);
                const uint32_t lane = tid & 63;
                const uint32_t tileBase = tile0 + ti * kExecTileBytes, p = tileBase + lane * 4;
                if (tileBase >= align16u(n))
                    break;   // uniform: the op ends before this tile
                {
                    const uint32_t nt = uni(h1.w);
                    const uint32_t mix = uni(h1.y);
                    const bool solo = nt <= kExecSolo;
                    const uint32_t c0 = wave == 0 ? load_cur(p, dst, n, valid) : 0u;
                    uint32_t acc0 = 0, acc1 = 0;
                    // wave w takes a contiguous share of the terms
                    const uint32_t a0 = solo ? 0 : nt * wave / kExecWaves;
                    const uint32_t a1 = solo ? (wave == 0 ? nt : 0) : nt * (wave + 1) / kExecWaves;
                    uint4 dv = make_uint4(0, 0, 0, 0);
                    gather(a0, a1, tileBase, p, acc0, acc1,
                           [&](uint32_t k, uint64_t& src, uint32_t& len, uint32_t& ca) {
                               const uint32_t j = (k - a0) & 63u;
                               if (j == 0) {
                                   const uint32_t idx = k + lane;
                                   dv = idx < a1 ? op_word(rb, seg, pos, kOpWords + idx) : make_uint4(0, 0, 0, 0);
                               }
                               lane_term(dv, j, src, len);
                               ca = rl(dv.w, j);
                               return true;
                           });
                    uint32_t out = acc0 ^ (mix > 1 ? gf_mul_dword(acc1, mix) : acc1);
                    if (!solo) {
                        if (wave != 0)
                            part[wave][0][lane] = out;
                        __syncthreads();
                        if (wave == 0) {
#pragma unroll
                            for (unsigned w = 1; w < kExecWaves; ++w)
                                out ^= part[w][0][lane];
                        }
                    }
                    if (wave == 0)
                        store_item(out, p, dst, n, valid, c0);
                    if (!solo && ti + 1 < nTiles)
                        __syncthreads();   // (part[] is written again for the next tile)
                }
            }
        } else if (kind == OP_ROWS) {
            // (specialised on whether the batch's whole block lies in the
            // LDS table: table_entry)
            auto rows_op = [&](auto fitTag) {
                constexpr bool Fit = decltype(fitTag)::value;
#ifdef SGPU_PHASE_CLOCKS
                unsigned long long tclk = clock64();
#endif
                const uint32_t R = n, E = valid, U = uni(h1.y);
                const uint32_t blk = pos + kOpWords;        // stream word of sum entry 0
                const uint32_t T = kRowSums + E;
                // the whole block (descriptors, updates, rows) to LDS: every
                // later header read is an LDS read, not a memory round trip
                const uint32_t blockWords = uni(h1.w);
                // (the host points the stage at the elements the batch reads:
                // GfOp.dst low word = stageLo, ops.h; the LDS table skips the
                // window entries below it: table_entry)
                const uint32_t stageLo = uni(h0.x) < E ? uni(h0.x) : E;
                for (uint32_t i = tid; i < kRowsTableLds; i += kExecThreads) {
                    const uint32_t word = i < kRowSums ? i : i + stageLo;
                    if (word < blockWords)
                        tableL[i] = op_word(rb, seg, pos, kOpWords + word);
                }
                if (tid == 0)
                    generalRows = 0;
                // the next op's prefetched block goes to the ring now (the ring's
                // other half is free: the previous op ended with a barrier), so
                // it holds no registers through the batch
                if (tid < kRingWords)
                    ring[cur ^ 1][tid] = pf;
                __syncthreads();
                PHASE_MARK(0, tclk);

                uint4 pre[kStagePre];   // the next tile's first stage entries (prefetched)
                for (uint32_t ti = 0; ti < nTiles; ++ti) {
                    // (lane-derived values re-derived per tile: hoisted out of the
                    // tile loop they would hold VGPRs through every phase)
                    const uint32_t tid = opaque(threadIdx.x);
                    const uint32_t lane = tid & 63;
                    const uint32_t tileBase = tile0 + ti * kExecTileBytes, p = tileBase + lane * 4;
                    // phase S: stage this tile of the 24 lane sums (slots 0..23, as
                    // they stand before the batch's updates) and of window elements
                    // [0, staged) (slots 24..): table entry x is stage slot x.  Thread
                    // t loads 16 bytes of entry t/16 per pass, four passes in flight;
                    // bytes past an entry's length (absent elements: all of them)
                    // read zero.
                    uint32_t span = 0;   // this sum's update: elements (lanes < 24 of wave 0)
                    const uint32_t staged = E - stageLo < stageCap ? E - stageLo : stageCap;
                    uint32_t from = 0, to = 0, usv = 0xffu;   // sum tid's update (lanes < 24 of wave 0)
                    if (ti == 0 && tid < kRowSums) {
                        // (at most one update per sum in a batch: Program::rows_update)
                        uint32_t found = 0xffu;
                        for (uint32_t u = 0; u < U; ++u) {
                            const uint4 w1 = table_entry<Fit>(tableL, seg, blk, kRowSums + E + u * kUpdateWords + 1, stageLo);
                            if (w1.z == tid && w1.y > w1.x) {
                                found = u;
                                from = w1.x;
                                to = w1.y;
                            }
                        }
                        if (found != 0xffu)
                            usv = table_entry<Fit>(tableL, seg, blk, kRowSums + E + found * kUpdateWords, stageLo).w >> 30;
                        updOfL[tid] = found;
                        updFromL[tid] = from;
                        updToL[tid] = to;
                        span = to > from ? (to - from + kLanes - 1) / kLanes : 0u;
                    }
                    if (ti == 0 && wave == 0) {
                        // (the longest update's element count)
                        uint32_t m = span;
#pragma unroll
                        for (unsigned d = 32; d >= 1; d >>= 1)
                            m = max(m, (uint32_t)__shfl_xor(m, d, 64));
                        // Lane mode: the three sums of every window lane l (k =
                        // 3l + s, coefficient 1 / CX / CX^2) are updated over one
                        // element range, all staged, or none of them is; each
                        // element is then read and split for the multiplies once
                        // for its three sums (a block-mode encoder's or decoder's
                        // batch)
                        const uint32_t k0 = lane < kRowSums ? lane - lane % kSums : 0u;
                        const uint32_t f0 = __shfl(from, k0, 64), t0 = __shfl(to, k0, 64);
                        const bool has = span != 0, has0 = __shfl(span, k0, 64) != 0;
                        bool ok = lane >= kRowSums ||
                                  (has == has0 && (!has || (from == f0 && to == t0 && usv == lane % kSums && from >= stageLo &&
                                                            from + (to - from - 1) / kLanes * kLanes - stageLo < staged)));
                        ok = __all(ok ? 1 : 0) != 0;
                        if (lane == 0) {
                            updSpanL = m;
                            laneModeL = (ok && m) ? 1u : 0u;
                        }
                    }
                    const uint32_t q16 = (tid & 15u) * 16u;         // byte within the tile
                    const bool sumsStaged = stageSlots >= kRowSums;
                    const uint32_t updWord = kOpWords + T;
                    const uint32_t rowWord = updWord + U * kUpdateWords;
                    const uint32_t planned = R < kPlanRows ? R : kPlanRows;
                    constexpr unsigned kPass = kExecThreads / 16;   // entries per pass
                    uint32_t* updAcc = &part[0][0][0];              // U <= 24 update accumulators of 64 dwords
                    static_assert(kExecWaves * 2 >= kRowSums, "update accumulators fit part[]");
                    for (uint32_t i = tid; i < U * 64; i += kExecThreads)
                        updAcc[i] = 0;
                    // rows [0, Rv) of a versioned batch (GfOp.dst high word, ops.h)
                    // take their corrections from corrL
                    const uint32_t Rv = min(min(uni(h0.y), R), (uint32_t)kVersionRows);
                    for (uint32_t i = tid; i < Rv * 128; i += kExecThreads)
                        (&corrL[0][0][0])[i] = 0;
                    if (tid == 0)
                        sumsDirty = 0;
                    const uint32_t entries = sumsStaged ? kRowSums + staged : 0u;
                    {
                        for (uint32_t x0 = tid / 16; x0 < entries; x0 += 4 * kPass) {
                            uint4 v[4];
                            // (a thread's first kStagePre entries of a later tile
                            // were fetched during the previous tile's rows)
                            const bool pref = ti > 0 && x0 < 4 * kPass;
#pragma unroll
                            for (unsigned u = 0; u < kStagePre; ++u)
                                v[u] = pre[u];
                            {
#pragma unroll
                                for (unsigned u = 0; u < 4; ++u) {
                                    const uint32_t x = x0 + u * kPass;
                                    if (pref && u < kStagePre)
                                        continue;
                                    v[u] = make_uint4(0, 0, 0, 0);
                                    if (x < entries) {
                                        const uint4 d =
                                            table_word<Fit>(tableL, seg, blk, x < kRowSums ? x : x + stageLo, stageLo);
                                        const uint64_t src = ((uint64_t)d.y << 32) | d.x;
                                        if (tileBase + q16 < d.z)
                                            v[u] = ld16(src + tileBase + q16);
                                    }
                                }
                            }
#pragma unroll
                            for (unsigned u = 0; u < 4; ++u) {
                                const uint32_t x = x0 + u * kPass;
                                if (x < entries)
                                    *reinterpret_cast<uint4*>(&stage[x * 64 + q16 / 4]) = v[u];
                            }
                        }
                    }
                    __syncthreads();
                    PHASE_MARK(1, tclk);

                    // phase A + B0: the lane-sum updates and the rows' term plans,
                    // dealt to the waves as units: unit < U*Q is part unit%Q of update
                    // unit/Q, the rest are row pairs of the plan.
                    //
                    // Updates (SiameseEncoder.cpp:359-418, SiameseDecoder.cpp:
                    // 1680-1739): element e = from, from+8, ... < to, coefficient 1, CX
                    // or CX^2 of its column.  Staged elements go four per wave
                    // instruction (quad g of the wave takes element 4j+g, lane l bytes
                    // 16*(l%16).., each lane with its element's multiply table from
                    // LDS); an update reaching past the stage falls back to the dword
                    // layout (lane j holds element j's descriptor and table, moved to
                    // scalars with readlane) with memory reads.  Partial sums meet in
                    // LDS accumulators (XOR atomics).
                    //
                    // Plan: row sizes are its selected sums plus one slot per LDPC
                    // draw, offsets a prefix sum over rows (every wave scans them all
                    // and keeps the rows whose pair it owns); the draws are made lane
                    // parallel, two rows per wave (lanes 32h.. take row 2i+h), and
                    // their reference source bytes counted; a row with a draw outside
                    // the staged window keeps reading memory (phase B1b).
                    //
                    // Version corrections (rows [0, Rv)): quad g of version task t
                    // takes lane sum 4t + g for every row; the sums of a row meet in
                    // corrL.
                    // Units x < vTasks are version tasks, then the update parts, then
                    // the row pairs.  Fewer than 16 version tasks own a wave each (the
                    // longest units, started first); the other waves share the rest.
                    const uint32_t vTasks = Rv ? kRowSums / 4 : 0u;
                    const uint32_t vWaves = vTasks < kExecWaves ? vTasks : 0u;
                    const uint32_t W2 = kExecWaves - vWaves;
                    // updates split into Q parts each, Q chosen for the fewest
                    // 16-element passes on the busiest wave (its parts of the
                    // longest update)
                    const bool laneMode = uni(laneModeL) != 0;
                    const uint32_t UL = laneMode ? (uint32_t)kLanes : U;   // update units before the split
                    uint32_t Q = 1;
                    if (UL) {
                        const uint32_t span = uni(updSpanL);   // (elements of the longest update)
                        uint32_t best = 0xffffffffu;
                        for (uint32_t q = 1; q <= 4; ++q) {
                            const uint32_t cost = ((UL * q + W2 - 1) / W2) * ((span + 16 * q - 1) / (16 * q));
                            if (cost < best) {
                                best = cost;
                                Q = q;
                            }
                        }
                    }
                    const uint32_t uUnits = UL * Q;
                    const uint32_t nPairs = sumsStaged ? (planned + 1) / 2 : 0u;
                    // (the row plans are the same for every tile: drawn for the first)
                    const uint32_t nUnits = vTasks + uUnits + (ti == 0 ? nPairs : 0u);
                    auto unit_wave = [&](uint32_t x) { return vWaves ? (x < vWaves ? x : vWaves + (x - vWaves) % W2) : x % kExecWaves; };
                    // the update this wave stores: its dst as kept, fetched now
                    uint64_t sdst = 0;
                    uint32_t sn = 0, svalid = 0, scur = 0;
                    if (wave < U) {
                        const uint4 w0 = table_entry<Fit>(tableL, seg, blk, updWord + wave * kUpdateWords - kOpWords, stageLo);
                        sdst = ((uint64_t)uni(w0.y) << 32) | uni(w0.x);
                        sn = uni(w0.z);
                        svalid = uni(w0.w) & 0x3fffffffu;
                        if (tileBase < align16u(sn))
                            scur = load_cur(p, sdst, sn, svalid);
                    }
                    if (ti == 0 && nPairs) {
                        uint32_t carry = 0;
                        for (uint32_t r0 = 0; r0 < planned; r0 += 64) {
                            const uint32_t r = r0 + lane;
                            uint32_t size = 0, n01 = 0;
                            if (r < planned) {
                                const uint4 w1 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 1 - kOpWords, stageLo);
                                // (a wide row reads its two k_ldpc sums as one pair)
                                const uint32_t pairs = (w1.x & kRowWide) ? 1u : (w1.w + kPairRate - 1) / kPairRate;
                                const uint32_t n0 = __builtin_popcount(w1.x & 0xffffffu) + pairs;
                                const uint32_t n1 = __builtin_popcount(w1.y & 0xffffffu) + pairs;
                                size = n0 + n1;
                                n01 = n0 | (n1 << 16);
                            }
                            uint32_t incl = size;
#pragma unroll
                            for (unsigned d = 1; d < 64; d <<= 1) {
                                const uint32_t t = __shfl_up(incl, d, 64);
                                if (lane >= d)
                                    incl += t;
                            }
                            const uint32_t offs = carry + incl - size;
                            if (r < planned && unit_wave(vTasks + uUnits + (r >> 1)) == wave) {
                                const bool fits = offs + size <= kPlanCap;
                                rowInfo[r] = make_uint2(fits ? offs : kNoPlan, n01);
                                if (!fits)
                                    generalRows = 1;
                            }
                            carry += __shfl(incl, 63, 64);
                        }
                    }
                    const uint32_t g = lane >> 4, b4 = (lane & 15u) * 4u;
                    if (wave == kExecWaves - 1) {
                        // rows whose cutoff is past every update's last element read
                        // the final sums as they are (no version corrections)
                        uint32_t m = 0;
                        if (lane < kRowSums && updOfL[lane] != 0xffu) {
                            const uint32_t f = updFromL[lane], t = updToL[lane];
                            m = f + ((t - f - 1) / kLanes) * kLanes + 1;
                        }
#pragma unroll
                        for (unsigned d = 16; d >= 1; d >>= 1)
                            m = max(m, (uint32_t)__shfl_xor(m, d, 64));
                        if (lane == 0)
                            updMaxLast1 = m;
                    }
                    PHASE_MARK(30, tclk);
                    const uint32_t xStep = vWaves ? (wave < vWaves ? nUnits : W2) : kExecWaves;
                    for (uint32_t x = vWaves && wave >= vWaves ? vTasks + wave - vWaves : wave; x < nUnits; x += xStep) {
                        const uint32_t unit = x - vTasks;   // (update parts, then row pairs)
                        if (x < vTasks) {
                            [[maybe_unused]] const unsigned long long vclk0 = PHASE_CLK();
                            // sum k's update elements as suffix sums: rows from the
                            // last (largest cutoff) down, each adding the elements
                            // in [its cutoff, the previous row's) and handing the
                            // suffix to the row if its masks select sum k (the rows'
                            // cutoffs never decrease: Program::rows_row)
                            const uint32_t k = 4 * x + g;
                            const uint32_t sidx = k % kSums;
                            const uint32_t p16 = tileBase + (lane & 15u) * 16u;
                            const uint32_t f = updFromL[k], t = updToL[k], slen = tableL[k].z;
                            const bool any = updOfL[k] != 0xffu && t > f && p16 < slen;
                            uint4 S = make_uint4(0, 0, 0, 0);
                            uint32_t hiE = t;
                            for (uint32_t r1 = Rv; r1 > 0; --r1) {
                                const uint32_t r = r1 - 1;
                                const uint4 w0 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords - kOpWords, stageLo);
                                const uint4 w1 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 1 - kOpWords, stageLo);
                                const uint32_t cut = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 2 - kOpWords, stageLo).y;
                                if (any) {
                                    const uint32_t first = cut <= f ? f : f + ((cut - f + kLanes - 1) / kLanes) * kLanes;
                                    for (uint32_t e = first; e < hiE; e += kLanes) {
                                        uint4 v = version_elem16<Fit>(e, p16, b4, stage, stageLo, staged, tableL, seg, blk);
                                        if (sidx != 0) {
                                            const uint32_t cx = cxL[win_entry<Fit>(tableL, seg, blk, e, stageLo).w %
                                                                    kColumnValuePeriod];
                                            v = gf_mul16_tab(v, gf_tab_l(permL, permC, sidx == 1 ? (cx & 0xffu) : (cx >> 8)));
                                        }
                                        S = xor16(S, v);
                                    }
                                    hiE = min(hiE, first);
                                }
                                const bool in0 = (w1.x >> k) & 1u, in1 = (w1.y >> k) & 1u;
                                if (any && (in0 || in1) && tileBase < align16u(w0.z) && (S.x | S.y | S.z | S.w)) {
                                    const uint4 V = p16 + 16 > slen ? mask16(S, (int)slen - (int)p16) : S;
                                    if (in0) {
                                        uint32_t* c0 = &corrL[r][0][b4];
                                        atomicXor(c0 + 0, V.x);
                                        atomicXor(c0 + 1, V.y);
                                        atomicXor(c0 + 2, V.z);
                                        atomicXor(c0 + 3, V.w);
                                    }
                                    if (in1) {
                                        uint32_t* c1 = &corrL[r][1][b4];
                                        atomicXor(c1 + 0, V.x);
                                        atomicXor(c1 + 1, V.y);
                                        atomicXor(c1 + 2, V.z);
                                        atomicXor(c1 + 3, V.w);
                                    }
                                }
                            }
                            PHASE_ADD(26, PHASE_CLK() - vclk0);
                            PHASE_ADD(29, 1);
                        } else if (unit < uUnits && laneMode) {
                            [[maybe_unused]] const unsigned long long uclk0 = PHASE_CLK();
                            // part unit%Q of window lane l's three sums: each element is
                            // read and split once, then XORed into sum 3l and
                            // multiplied by its column's CX / CX^2 into 3l+1 / 3l+2
                            // (SiameseEncoder.cpp:359-418; all staged: lane mode)
                            const uint32_t l = unit / Q, uq = unit % Q;
                            const uint32_t ua = uni(updOfL[kSums * l]), ub = uni(updOfL[kSums * l + 1]),
                                           uc = uni(updOfL[kSums * l + 2]);
                            const uint32_t from = uni(updFromL[kSums * l]), to = uni(updToL[kSums * l]);
                            const uint32_t total = to > from ? (to - from + kLanes - 1) / kLanes : 0;
                            const uint32_t k0 = total * uq / Q, k1 = total * (uq + 1) / Q;
                            if (ua != 0xffu && k0 < k1) {
                                auto live = [&](uint32_t u) {
                                    return tileBase <
                                           align16u(uni(table_entry<Fit>(tableL, seg, blk, updWord + u * kUpdateWords - kOpWords,
                                                                         stageLo).z));
                                };
                                const bool la = live(ua), lb = live(ub), lc = live(uc);
                                if (la || lb || lc) {
                                    uint32_t refBytes = 0;
                                    uint4 A0 = make_uint4(0, 0, 0, 0), A1 = A0, A2 = A0;
                                    for (uint32_t kk = k0; kk < k1; kk += 4) {
                                        const uint32_t k = kk + g;
                                        const bool act = k < k1;
                                        const uint32_t e = from + (act ? k : k0) * kLanes;
                                        const uint4 ev = win_entry<Fit>(tableL, seg, blk, e, stageLo);
                                        if (act && (lane & 15u) == 0)
                                            refBytes += ev.z;
                                        const uint32_t cx = cxL[ev.w % kColumnValuePeriod];   // CX | CX^2 << 8
                                        const uint4 v = lds16(stage, (act ? kRowSums + e - stageLo : zeroSlot) * 64 + b4);
                                        const GfTab t1 = gf_tab_l(permL, permC, cx & 0xffu);
                                        const GfTab t2 = gf_tab_l(permL, permC, cx >> 8);
                                        const Split16 sp = gf_split16(v);
                                        A0 = xor16(A0, v);
                                        A1 = xor16(A1, gf_mul16_split(sp, t1));
                                        A2 = xor16(A2, gf_mul16_split(sp, t2));
                                    }
                                    // (the quads hold different elements: each adds its share)
                                    if (la) {
                                        atomicXor(&updAcc[ua * 64 + b4 + 0], A0.x);
                                        atomicXor(&updAcc[ua * 64 + b4 + 1], A0.y);
                                        atomicXor(&updAcc[ua * 64 + b4 + 2], A0.z);
                                        atomicXor(&updAcc[ua * 64 + b4 + 3], A0.w);
                                    }
                                    if (lb) {
                                        atomicXor(&updAcc[ub * 64 + b4 + 0], A1.x);
                                        atomicXor(&updAcc[ub * 64 + b4 + 1], A1.y);
                                        atomicXor(&updAcc[ub * 64 + b4 + 2], A1.z);
                                        atomicXor(&updAcc[ub * 64 + b4 + 3], A1.w);
                                    }
                                    if (lc) {
                                        atomicXor(&updAcc[uc * 64 + b4 + 0], A2.x);
                                        atomicXor(&updAcc[uc * 64 + b4 + 1], A2.y);
                                        atomicXor(&updAcc[uc * 64 + b4 + 2], A2.z);
                                        atomicXor(&updAcc[uc * 64 + b4 + 3], A2.w);
                                    }
                                    // (reference bytes: one add / muladd per original and sum)
                                    if (tileBase == 0)
                                        acct_wave(&acctL, refBytes * ((la ? 1u : 0u) + (lb ? 1u : 0u) + (lc ? 1u : 0u)));
                                }
                            }
                            PHASE_ADD(19, PHASE_CLK() - uclk0);
                            PHASE_ADD(27, 1);
                        } else if (unit < uUnits) {
                            [[maybe_unused]] const unsigned long long uclk0 = PHASE_CLK();
                            const uint32_t u = unit / Q;
                            const uint32_t uq = unit % Q;
                            const uint4 w0 = table_entry<Fit>(tableL, seg, blk, updWord + u * kUpdateWords - kOpWords, stageLo);
                            const uint4 w1 = table_entry<Fit>(tableL, seg, blk, updWord + u * kUpdateWords + 1 - kOpWords, stageLo);
                            const uint32_t un = uni(w0.z), us = uni(w0.w) >> 30;
                            const uint32_t from = uni(w1.x), to = uni(w1.y);
                            const uint32_t total = to > from ? (to - from + kLanes - 1) / kLanes : 0;
                            const uint32_t k0 = total * uq / Q, k1 = total * (uq + 1) / Q;
                            if (tileBase < align16u(un) && k0 < k1) {
                                uint32_t refBytes = 0;   // reference source bytes (one add/muladd per original)
                                if (from + k0 * kLanes >= stageLo && from + (k1 - 1) * kLanes - stageLo < staged) {
                                    // quad layout, four elements per quad in flight
                                    // (elements past the range read the zero slot)
                                    uint4 a = make_uint4(0, 0, 0, 0);
                                    for (uint32_t kk = k0; kk < k1; kk += 16) {
                                        uint32_t slot[4], y[4];
#pragma unroll
                                        for (unsigned j = 0; j < 4; ++j) {
                                            const uint32_t k = kk + 4 * j + g;
                                            const bool act = k < k1;
                                            const uint32_t e = from + (act ? k : k0) * kLanes;
                                            const uint4 ev = win_entry<Fit>(tableL, seg, blk, e, stageLo);
                                            if (act && (lane & 15u) == 0)
                                                refBytes += ev.z;
                                            slot[j] = act ? kRowSums + e - stageLo : zeroSlot;
                                            const uint32_t cx = cxL[ev.w % kColumnValuePeriod];   // CX, CX^2
                                            y[j] = us == 1 ? (cx & 0xff) : (cx >> 8);
                                        }
                                        uint4 v[4];
#pragma unroll
                                        for (unsigned j = 0; j < 4; ++j)
                                            v[j] = lds16(stage, slot[j] * 64 + b4);
                                        if (us != 0) {
                                            // (the four tables read before any multiply: one
                                            // LDS round trip, not four)
                                            GfTab tb[4];
#pragma unroll
                                            for (unsigned j = 0; j < 4; ++j)
                                                tb[j] = gf_tab_l(permL, permC, y[j]);
                                            __builtin_amdgcn_sched_barrier(0);   // (keep the reads together)
#pragma unroll
                                            for (unsigned j = 0; j < 4; ++j)
                                                v[j] = gf_mul16_tab(v[j], tb[j]);
                                        }
                                        a = xor5_16(a, v[0], v[1], v[2], v[3]);
                                    }
                                    atomicXor(&updAcc[u * 64 + b4 + 0], a.x);
                                    atomicXor(&updAcc[u * 64 + b4 + 1], a.y);
                                    atomicXor(&updAcc[u * 64 + b4 + 2], a.z);
                                    atomicXor(&updAcc[u * 64 + b4 + 3], a.w);
                                } else {
                                    uint32_t acc = 0;
                                    for (uint32_t c = k0; c < k1; c += 64) {
                                        const uint32_t e = from + (c + lane) * kLanes;
                                        const uint4 ev = c + lane < k1 ? win_entry<Fit>(tableL, seg, blk, e, stageLo)
                                                                       : make_uint4(0, 0, 0, 0);
                                        const uint32_t cx = cxL[ev.w % kColumnValuePeriod];   // CX, CX^2
                                        const GfTab tab = gf_tab_l(permL, permC, us == 1 ? (cx & 0xff) : (cx >> 8));
                                        refBytes += ev.z;
                                        const uint32_t cnt = k1 - c < 64 ? k1 - c : 64;
                                        for (uint32_t j0 = 0; j0 < cnt; j0 += 16) {
                                            uint32_t v[16];
#pragma unroll
                                            for (unsigned k = 0; k < 16; ++k) {
                                                const uint32_t j = j0 + k;
                                                const uint32_t ej = from + (c + j) * kLanes;
                                                v[k] = 0;
                                                if (j < cnt) {
                                                    if (ej - stageLo < staged) {
                                                        v[k] = stage[(kRowSums + ej - stageLo) * 64 + lane];
                                                    } else {
                                                        uint64_t src;
                                                        uint32_t len;
                                                        lane_term(ev, j, src, len);
                                                        if (tileBase < len)
                                                            v[k] = term_load(src, len, p);
                                                    }
                                                }
                                            }
#pragma unroll
                                            for (unsigned k = 0; k < 16; ++k) {
                                                const uint32_t j = j0 + k;
                                                if (j < cnt) {
                                                    if (us == 0) {
                                                        acc ^= v[k];
                                                    } else {
                                                        const GfTab t{rl(tab.a0, j), rl(tab.a1, j), rl(tab.b0, j),
                                                                      rl(tab.b1, j), rl(tab.c, j)};
                                                        acc ^= gf_mul_tab(v[k], t);
                                                    }
                                                }
                                            }
                                        }
                                    }
                                    atomicXor(&updAcc[u * 64 + lane], acc);
                                }
                                if (tileBase == 0)
                                    acct_wave(&acctL, refBytes);
                            }
                            PHASE_ADD(19, PHASE_CLK() - uclk0);
                            PHASE_ADD(27, 1);
                        } else {
                            [[maybe_unused]] const unsigned long long pclk0 = PHASE_CLK();
                            const uint32_t h = lane >> 5, hl = lane & 31u;
                            const uint32_t r = 2 * (unit - uUnits) + h;
                            const uint2 info = r < planned ? rowInfo[r] : make_uint2(kNoPlan, 0u);   // (own write)
                            const bool act = info.x != kNoPlan;
                            if (!__any(act ? 1 : 0))
                                continue;
                            const uint4 z4 = make_uint4(0, 0, 0, 0);
                            const uint4 w0 = act ? table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords - kOpWords, stageLo) : z4;
                            const uint4 w1 = act ? table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 1 - kOpWords, stageLo) : z4;
                            const uint4 w2 = act ? table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 2 - kOpWords, stageLo) : z4;
                            const uint32_t rn = w0.z;
                            const uint32_t m0 = w1.x & 0xffffffu, m1 = w1.y & 0xffffffu;
                            const uint32_t row = w1.z, N = act ? w1.w : 0u, woff = w2.x;
                            const uint32_t off0 = info.x, off1 = info.x + (info.y & 0xffffu);
                            const uint32_t pc0 = __builtin_popcount(m0), pc1 = __builtin_popcount(m1);
                            // sums: lane k < 24 of the half places slot k if its bit is set
                            if (act && hl < kRowSums) {
                                const uint32_t below = (1u << hl) - 1u;
                                if (m0 >> hl & 1u)
                                    plan[off0 + __builtin_popcount(m0 & below)] = (uint16_t)hl;
                                if (m1 >> hl & 1u)
                                    plan[off1 + __builtin_popcount(m1 & below)] = (uint16_t)hl;
                            }
                            // draws: even -> row list, odd -> product list; a wide
                            // row's two "draws" are its k_ldpc sums L0 / L1 at
                            // window entries woff, woff + 1 (counted by k_ldpc)
                            const bool wide = act && (w1.x & kRowWide) != 0;
                            const uint32_t D = N ? 2 * ((N + kPairRate - 1) / kPairRate) : (wide ? 2u : 0u);
                            uint32_t Dmax = max(D, (uint32_t)__shfl_xor(D, 32, 64));
                            Dmax = uni(Dmax);
                            bool general = false;
                            uint32_t refBytes = 0;
                            const uint64_t inc = ((uint64_t)row << 1) | 1u;
                            uint64_t sc = (inc + N) * kPcgMul + inc;   // state after Seed()
                            // x % N through a double reciprocal: the quotient estimate
                            // is within one for 32-bit x, then corrected exactly
                            const double invN = N ? 1.0 / (double)N : 0.0;
                            // (an opaque lane index keeps these loads in the loop: hoisted
                            // out of the op loop they would hold 4 VGPRs through every phase)
                            const uint32_t jl = opaque(hl);
                            const uint64_t ja = c_pcgA[jl], jg = c_pcgG[jl];
                            for (uint32_t c = 0; c < Dmax; c += 32) {
                                const uint32_t d = c + hl;
                                const uint64_t st = ja * sc + inc * jg;
                                sc = c_pcgA[32] * sc + inc * c_pcgG[32];
                                if (d < D) {
                                    uint32_t e = woff + d;
                                    if (!wide) {
                                        const uint32_t x = pcg_output(st);
                                        const uint32_t qn = (uint32_t)((double)x * invN);
                                        int64_t rr = (int64_t)x - (int64_t)qn * N;
                                        rr = rr < 0 ? rr + N : (rr >= (int64_t)N ? rr - N : rr);
                                        e = woff + (uint32_t)rr;
                                    }
                                    const uint32_t len = win_entry<Fit>(tableL, seg, blk, e, stageLo).z;
                                    if (!wide)
                                        refBytes += len < rn ? len : rn;
                                    general |= e - stageLo >= staged;
                                    const uint32_t at = (d & 1u) ? off1 + pc1 + d / 2 : off0 + pc0 + d / 2;
                                    plan[at] = (uint16_t)(e - stageLo < staged ? kRowSums + e - stageLo : 0);
                                }
                            }
                            if (tileBase == 0)
                                acct_wave(&acctL, refBytes);
                            const uint64_t gb = __ballot(general ? 1 : 0);
                            if (hl == 0 && act && (uint32_t)(gb >> (32 * h)) != 0) {
                                rowInfo[r].x = kPlanGeneral;
                                generalRows = 1;
                            }
                            PHASE_ADD(20, PHASE_CLK() - pclk0);
                            PHASE_ADD(28, 1);
                        }
                    }
                    PHASE_MARK(31, tclk);
                    __syncthreads();
                    PHASE_MARK(2, tclk);

                    // update stores.  Update u's sum (SumUpdate.sum = k)
                    // also refreshes stage slot k straight from registers when it is
                    // the buffer the rows read and the stored bytes cover the staged
                    // ones; anything else marks the stage stale and the sums are
                    // re-read from memory after a barrier.
                    for (uint32_t u = wave; u < U; u += kExecWaves) {
                        const uint4 w0 = table_entry<Fit>(tableL, seg, blk, updWord + u * kUpdateWords - kOpWords, stageLo);
                        const uint4 w1 = table_entry<Fit>(tableL, seg, blk, updWord + u * kUpdateWords + 1 - kOpWords, stageLo);
                        const uint64_t udst = ((uint64_t)uni(w0.y) << 32) | uni(w0.x);
                        const uint32_t un = uni(w0.z), uvalid = uni(w0.w) & 0x3fffffffu;
                        if (tileBase >= align16u(un))
                            continue;   // (this tile of the sum is unchanged, as staged)
                        const uint32_t cu = u == wave ? scur : load_cur(p, udst, un, uvalid);
                        const uint32_t out = item_value(updAcc[u * 64 + lane], p, un, uvalid, cu);
                        if (p < align16u(un))
                            st4(udst + p, out);
                        // (slot k holds the buffer the rows read as sum k; an update of
                        // another buffer -- the rows of this batch do not read the sum,
                        // it grew after they took their table -- leaves it as staged)
                        const uint32_t k = uni(w1.z);
                        bool stale = k >= kRowSums;
                        if (k < kRowSums && sumsStaged) {
                            const uint4 d = tableL[k];
                            const uint64_t src = ((uint64_t)uni(d.y) << 32) | uni(d.x);
                            const uint32_t len = uni(d.z);
                            if (src == udst) {
                                // (exactly the sum's first `len` bytes, as the rows read
                                // it: with versioned reads the update may have grown it)
                                if (align16u(len) <= align16u(un))
                                    stage[k * 64 + lane] = p < len ? out & byte_mask((int)len - (int)p) : 0u;
                                else
                                    stale = true;
                            }
                        }
                        if (stale && nPairs && lane == 0)   // (no plan: no row reads the stage)
                            sumsDirty = 1;
                    }
                    __syncthreads();
                    PHASE_MARK(3, tclk);
                    if (tid == 0)
                        PHASE_ADD(21, sumsDirty ? 1 : 0);
                    if (sumsStaged && uni(sumsDirty)) {
                        // (this workgroup's own stores, visible after the barrier)
                        if (tid < kRowSums * 16) {
                            const uint32_t k = tid / 16;
                            const uint4 d = tableL[k];
                            const uint64_t src = ((uint64_t)d.y << 32) | d.x;
                            uint4 v = make_uint4(0, 0, 0, 0);
                            if (tileBase + q16 < d.z)
                                v = mask16(ld16(src + tileBase + q16), (int)d.z - (int)(tileBase + q16));
                            *reinterpret_cast<uint4*>(&stage[k * 64 + q16 / 4]) = v;
                        }
                        __syncthreads();
                    }
                    PHASE_MARK(4, tclk);
                    if (ti + 1 < nTiles) {
                        // the next tile's first kStagePre stage entries per thread, in
                        // flight through this tile's rows (its bytes are untouched
                        // until its own phases: every op is byte-column local)
                        const uint32_t nb = tileBase + kExecTileBytes;
#pragma unroll
                        for (unsigned u = 0; u < kStagePre; ++u) {
                            const uint32_t x = tid / 16 + u * kPass;
                            pre[u] = make_uint4(0, 0, 0, 0);
                            if (x < entries) {
                                const uint4 d = table_word<Fit>(tableL, seg, blk, x < kRowSums ? x : x + stageLo, stageLo);
                                const uint64_t src = ((uint64_t)d.y << 32) | d.x;
                                if (nb + q16 < d.z)
                                    pre[u] = ld16(src + nb + q16);
                            }
                        }
                    }

                    // phase B1a: planned rows, four per wave at a time: quad g of the
                    // wave (lanes 16g..16g+15) takes row 4t+g, and lane l holds bytes
                    // 16*(l%16).. of the tile, so one 16-byte LDS read per lane moves
                    // one term of each of four rows and every per-row step (the
                    // descriptors, the RX product, the stores) is paid once per four
                    // rows.
                    {
                        const uint32_t nq = (planned + 3) / 4;
                        const uint32_t g = lane >> 4, b4 = (lane & 15u) * 4u;
                        const uint32_t p16 = tileBase + (lane & 15u) * 16u;
                        for (uint32_t task = wave; task < nq; task += kExecWaves) {
#ifdef SGPU_PHASE_CLOCKS
                            unsigned long long qclk = clock64();
#endif
                            const uint32_t r = task * 4 + g;
                            const uint2 info = r < planned ? rowInfo[r] : make_uint2(kNoPlan, 0u);
                            const bool act = info.x < kPlanGeneral;
                            if (!__any(act ? 1 : 0))
                                continue;
                            const uint4 z4 = make_uint4(0, 0, 0, 0);
                            const uint4 w0 = act ? table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords - kOpWords, stageLo) : z4;
                            const uint4 w1 = act ? table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 1 - kOpWords, stageLo) : z4;
                            const uint4 w2 = act ? table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 2 - kOpWords, stageLo) : z4;
                            const uint64_t rdst = ((uint64_t)w0.y << 32) | w0.x;
                            const uint32_t rn = w0.z, rvalid = w0.w;
                            const uint32_t mix = w1.y >> 24;
                            const bool live = act && tileBase < align16u(rn);
                            // dst as kept (decoder rows), fetched before the terms stream in
                            const uint4 cur = live ? load_cur16(p16, rdst, rn, rvalid) : z4;
                            const GfTab tab = gf_tab_l(permL, permC, mix > 1 ? mix : 1u);
                            const uint32_t off0 = info.x, n0 = live ? (info.y & 0xffffu) : 0u;
                            const uint32_t off1 = info.x + (info.y & 0xffffu), n1 = live ? (info.y >> 16) : 0u;
                            uint32_t most = n0 > n1 ? n0 : n1;
                            most = max(most, (uint32_t)__shfl_xor(most, 16, 64));
                            most = uni(max(most, (uint32_t)__shfl_xor(most, 32, 64)));
                            PHASE_MARK(13, qclk);
                            uint4 a0 = z4, a1 = z4;
                            // 16 terms at a time: lane i of a quad reads plan entry
                            // t+i of its row's lists, a row broadcast (DPP) hands
                            // entry j to the whole quad, 4 terms of each list in flight
                            // (no masking after the reads, so they go out together)
                            const char* lb = reinterpret_cast<const char*>(stage) + b4 * 4u;   // (this lane's 16 bytes)
                            for (uint32_t t = 0; t < most; t += 16) {
                                const uint32_t i = t + (lane & 15u);
                                // (entries past a list's end name the zero slot)
                                const uint32_t s0 = i < n0 ? (uint32_t)plan[off0 + i] : zeroSlot;
                                const uint32_t s1 = i < n1 ? (uint32_t)plan[off1 + i] : zeroSlot;
                                // (byte offsets of the slots, so a term's address is one
                                // v_add with the row broadcast folded in as its DPP source)
                                const uint32_t s0b = s0 * (64u * 4u), s1b = s1 * (64u * 4u);
                                const uint32_t left = most - t;   // (uniform)
#define SGPU_TERM(S, K) (*reinterpret_cast<const uint4*>(lb + row_bcast<(K)>(S)))
#define SGPU_QUAD_GROUP(J)                                                                                  \
            {                                                                                                       \
                const uint4 x0 = SGPU_TERM(s0b, (J));                                                               \
                const uint4 x1 = SGPU_TERM(s0b, (J) + 1);                                                           \
                const uint4 x2 = SGPU_TERM(s0b, (J) + 2);                                                           \
                const uint4 x3 = SGPU_TERM(s0b, (J) + 3);                                                           \
                const uint4 y0 = SGPU_TERM(s1b, (J));                                                               \
                const uint4 y1 = SGPU_TERM(s1b, (J) + 1);                                                           \
                const uint4 y2 = SGPU_TERM(s1b, (J) + 2);                                                           \
                const uint4 y3 = SGPU_TERM(s1b, (J) + 3);                                                           \
                a0 = xor5_16(a0, x0, x1, x2, x3);                                                                   \
                a1 = xor5_16(a1, y0, y1, y2, y3);                                                                   \
            }
                                SGPU_QUAD_GROUP(0)
                                if (left > 4)
                                    SGPU_QUAD_GROUP(4)
                                if (left > 8)
                                    SGPU_QUAD_GROUP(8)
                                if (left > 12)
                                    SGPU_QUAD_GROUP(12)
#undef SGPU_TERM
#undef SGPU_QUAD_GROUP
                            }
                            PHASE_MARK(14, qclk);
                            // (rows read the sums as of their cutoff, ops.h RowItem)
                            if (r < Rv) {
                                a0 = xor16(a0, lds16(&corrL[r][0][0], b4));
                                a1 = xor16(a1, lds16(&corrL[r][1][0], b4));
                            }
                            if (__any(act && r >= Rv && w2.y < updMaxLast1 ? 1 : 0)) {
                                row_versions16<Fit>(w1.x & 0xffffffu, w1.y & 0xffffffu, w2.y, live && r >= Rv, p16, b4, updOfL, updFromL,
                                               updToL, cxL, permL, permC, stage, stageLo, staged, tableL, seg, blk, a0, a1);
                                PHASE_MARK(16, qclk);
                                if (lane == 0)
                                    PHASE_ADD(17, 1);
                            }
                            if (live)
                                store_item16(xor16(a0, gf_mul16_tab(a1, tab)), p16, rdst, rn, rvalid, cur);
                            if (act) {
                                store_literal(p16, rdst, rn, row_lit_len(w1.x), w2.z, w2.w, 16);
                            }
                            PHASE_MARK(15, qclk);
                        }
                    }

                    // phase B1b: rows without a plan (a draw outside the staged
                    // window, or past the plan's capacity).  R >= W: wave w takes rows
                    // w, w+W, ...; R < W: row r's terms are split into P = W / R parts,
                    // unit w = (w / P, w % P), and the parts meet in LDS.  They read
                    // sums and undrawn-from-LDS picks from memory; lane j < 24 holds
                    // sum entry j.
                    const uint4 sumv = lane < kRowSums ? tableL[lane] : make_uint4(0, 0, 0, 0);
                    const uint32_t P = R >= kExecWaves ? 1u : kExecWaves / R;
                    const uint32_t units = (R > planned || uni(generalRows)) ? (P == 1 ? R : R * P) : 0u;
                    for (uint32_t unit = wave; unit < units; unit += kExecWaves) {
                        const uint32_t r = P == 1 ? unit : unit / P;
                        const uint32_t q = P == 1 ? 0 : unit % P;
                        const uint4 w0 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords - kOpWords, stageLo);
                        const uint4 w1 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 1 - kOpWords, stageLo);
                        const uint4 w2 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 2 - kOpWords, stageLo);
                        const uint64_t rdst = ((uint64_t)uni(w0.y) << 32) | uni(w0.x);
                        const uint32_t rn = uni(w0.z), rvalid = uni(w0.w);
                        const uint32_t m0 = uni(w1.x), m1 = uni(w1.y), row = uni(w1.z), N = uni(w1.w);
                        const uint32_t off = uni(w2.x);
                        const uint32_t mix = m1 >> 24;
                        const uint2 info = r < planned ? rowInfo[r] : make_uint2(kNoPlan, 0u);
                        const uint32_t pinfo = uni(info.x);
                        if (pinfo < kPlanGeneral)
                            continue;   // (phase B1a)
#ifdef SGPU_PHASE_CLOCKS
                        unsigned long long rclk = clock64();
#endif
                        // dst as kept (decoder rows) and the product's multiply table,
                        // fetched before the terms stream in
                        const uint32_t c0 = (P == 1 && tileBase < align16u(rn)) ? load_cur(p, rdst, rn, rvalid) : 0u;
                        const GfTab mixTab = gf_tab_l(permL, permC, mix);
                        uint32_t acc0 = 0, acc1 = 0;
                        if (tileBase < align16u(rn)) {
                            // dense part (part 0): the sums the opcodes select (bit
                            // lane*3+s; mask1 feeds the product)
                            if (q == 0) {
                                uint64_t bits = (uint64_t)(m0 & 0xffffffu) | ((uint64_t)(m1 & 0xffffffu) << 24);
                                gather<true>(0, (uint32_t)__builtin_popcountll(bits), tileBase, p, acc0, acc1,
                                       [&](uint32_t, uint64_t& src, uint32_t& len, uint32_t& ca) {
                                           const uint32_t b = (uint32_t)__builtin_ctzll(bits);
                                           bits &= bits - 1;
                                           const uint32_t k = b < kRowSums ? b : b - kRowSums;
                                           lane_term(sumv, k, src, len);
                                           ca = 1u | ((b >= kRowSums ? 1u : 0u) << 8);
                                           return len != 0;
                                       });
                                // (the sums as of the row's cutoff, ops.h RowItem)
                                if (r < Rv) {
                                    acc0 ^= corrL[r][0][lane];
                                    acc1 ^= corrL[r][1][lane];
                                } else if (uni(w2.y) < updMaxLast1)
                                    row_versions4<Fit>(m0 & 0xffffffu, m1 & 0xffffffu, uni(w2.y), tileBase, p, lane, updOfL, updFromL,
                                              updToL, cxL, stage, stageLo, staged, tableL, seg, blk, acc0, acc1);
                            }
                            // sparse part: this unit's share of the 2*ceil(N/16) draws
                            // (pairs stay whole: even draw -> row, odd -> product)
                            if ((m0 & kRowWide) && q == 0) {
                                // a wide row's k_ldpc sums L0 -> acc0, L1 -> acc1
#pragma unroll
                                for (uint32_t k = 0; k < 2; ++k) {
                                    const uint32_t e = off + k;
                                    uint32_t v = 0;
                                    if (e - stageLo < staged) {
                                        v = stage[(kRowSums + e - stageLo) * 64 + lane];
                                    } else {
                                        const uint4 ev = win_entry<Fit>(tableL, seg, blk, e, stageLo);
                                        const uint64_t src = ((uint64_t)uni(ev.y) << 32) | uni(ev.x);
                                        const uint32_t len = uni(ev.z);
                                        if (tileBase < len)
                                            v = term_load(src, len, p);
                                    }
                                    if (k == 0)
                                        acc0 ^= v;
                                    else
                                        acc1 ^= v;
                                }
                            }
                            if (N != 0) {
                                const uint32_t pairs = (N + kPairRate - 1) / kPairRate;
                                const uint32_t d0 = 2 * (pairs * q / P), d1 = 2 * (pairs * (q + 1) / P);
                                const uint32_t refBytes = row_picks<Fit>(row, N, off, d0, d1, rn, tileBase, p, lane,
                                                                    c_pcgA[opaque(lane)], c_pcgG[opaque(lane)], stage, stageLo, staged, tableL, seg, blk, acc0, acc1);
                                // (a planned row's draws were counted by its plan)
                                if (pinfo == kNoPlan && tileBase == 0 && lane == 0 && refBytes)
                                    atomicAdd(&acctL, (unsigned long long)refBytes);
                            }
                        }
                        if (P > 1) {
                            part[wave][0][lane] = acc0;
                            part[wave][1][lane] = acc1;
                        } else {
                            if (tileBase < align16u(rn))
                                store_item(acc0 ^ (mix > 1 ? gf_mul_tab(acc1, mixTab) : acc1), p, rdst, rn, rvalid, c0);
                            PHASE_MARK(18, rclk);
                            PHASE_ADD(23, 1);
                            store_literal(p, rdst, rn, row_lit_len(m0), uni(w2.z), uni(w2.w));
                            PHASE_MARK(22, rclk);
                        }
                    }
                    if (P > 1 && units) {
                        __syncthreads();
                        if (wave < units && wave % P == 0 &&
                            !(wave / P < planned && uni(rowInfo[wave / P].x) < kPlanGeneral)) {
                            const uint32_t r = wave / P;
                            const uint4 w0 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords - kOpWords, stageLo);
                            const uint4 w1 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 1 - kOpWords, stageLo);
                            const uint4 w2 = table_entry<Fit>(tableL, seg, blk, rowWord + r * kRowWords + 2 - kOpWords, stageLo);
                            const uint64_t rdst = ((uint64_t)uni(w0.y) << 32) | uni(w0.x);
                            const uint32_t rn = uni(w0.z), rvalid = uni(w0.w);
                            const uint32_t m0 = uni(w1.x), mix = uni(w1.y) >> 24;
                            uint32_t acc0 = 0, acc1 = 0;
                            for (uint32_t k = 0; k < P; ++k) {
                                acc0 ^= part[wave + k][0][lane];
                                acc1 ^= part[wave + k][1][lane];
                            }
                            if (tileBase < align16u(rn)) {
                                const uint32_t c0 = load_cur(p, rdst, rn, rvalid);
                                store_item(acc0 ^ (mix > 1 ? gf_mul_dword(acc1, mix) : acc1), p, rdst, rn, rvalid, c0);
                            }
                            store_literal(p, rdst, rn, row_lit_len(m0), uni(w2.z), uni(w2.w));
                        }
                    }
                    if (ti + 1 < nTiles)
                        __syncthreads();   // (the stage, plans' readers and part[] turn over)
                }
                PHASE_MARK(5, tclk);
                if (tid == 0) {
#ifdef SGPU_PHASE_CLOCKS
                    t5 = clock64();
                    atomicAdd(&g_phaseClk[8], 1ull);
                    atomicAdd(&g_phaseClk[9], (unsigned long long)R);
                    atomicAdd(&g_phaseClk[10], (unsigned long long)U);
                    atomicAdd(&g_phaseClk[11], (unsigned long long)E);
                    atomicAdd(&g_phaseClk[12], (unsigned long long)(E - stageLo < stageCap ? E - stageLo : stageCap));
#endif
                }
            };
            {
                const uint32_t lo = uni(h0.x) < valid ? uni(h0.x) : valid;   // (stageLo)
                if (uni(h1.w) <= kRowsTableLds + lo)
                    rows_op(std::true_type{});
                else
                    rows_op(std::false_type{});
            }
        } else if (kind == OP_LINCOMBS) {
            // independent combinations, whole items per wave: each wave
            // streams its item's terms (kExecDepth loads in flight) and
            // stores it, no barrier until the batch ends
            for (uint32_t k = wave; k < n; k += kExecWaves) {
                const uint32_t iw = kOpWords + k * kLcWords;
                const uint4 w0 = op_word(rb, seg, pos, iw);
                const uint4 w1 = op_word(rb, seg, pos, iw + 1);
                const uint64_t idst = ((uint64_t)uni(w0.y) << 32) | uni(w0.x);
                const uint32_t in = uni(w0.z), ivalid = uni(w0.w);
                const uint32_t ts = uni(w1.x), tc = uni(w1.y), mixLit = uni(w1.z);
                const uint32_t imix = mixLit & 0xffu, litLen = (mixLit >> 8) & 0xffu;
                for (uint32_t ti = 0; ti < nTiles; ++ti) {
                    const uint32_t tileBase = tile0 + ti * kExecTileBytes, p = tileBase + lane * 4;
                    if (tileBase < align16u(in)) {   // uniform: the item reaches this tile
                        const uint32_t c0 = load_cur(p, idst, in, ivalid);
                        uint32_t acc0 = 0, acc1 = 0;
                        uint4 dv = make_uint4(0, 0, 0, 0);
                        gather(0, tc, tileBase, p, acc0, acc1,
                               [&](uint32_t t, uint64_t& src, uint32_t& len, uint32_t& ca) {
                                   const uint32_t j = t & 63u;
                                   if (j == 0) {
                                       const uint32_t idx = t + lane;
                                       dv = idx < tc ? op_word(rb, seg, pos, kOpWords + ts + idx)
                                                     : make_uint4(0, 0, 0, 0);
                                   }
                                   lane_term(dv, j, src, len);
                                   ca = rl(dv.w, j);
                                   return true;
                               });
                        store_item(acc0 ^ (imix > 1 ? gf_mul_dword(acc1, imix) : acc1), p, idst, in, ivalid, c0);
                    }
                    if (litLen) {
                        // the footer after its combination (same lanes, in order)
                        const uint4 w2 = op_word(rb, seg, pos, iw + 2);
                        store_literal(p, idst, uni(w1.w), litLen, uni(w2.x), uni(w2.y));
                    }
                }
            }
        } else if (kind == OP_COPIES) {
            // kCopyBatch copies per wave at a time over kCopyTiles tiles, all
            // their loads in flight before the first store; sources carry
            // their zero tails
            constexpr unsigned kCopyBatch = 4, kCopyTiles = 4;
            for (uint32_t k0 = wave * kCopyBatch; k0 < n; k0 += kExecWaves * kCopyBatch) {
                uint64_t d[kCopyBatch], sr[kCopyBatch];
                uint32_t l[kCopyBatch];
#pragma unroll
                for (unsigned u = 0; u < kCopyBatch; ++u) {
                    d[u] = sr[u] = 0;
                    l[u] = 0;
                    if (k0 + u < n) {
                        const uint4 w0 = op_word(rb, seg, pos, kOpWords + (k0 + u) * kCopyWords);
                        const uint4 w1 = op_word(rb, seg, pos, kOpWords + (k0 + u) * kCopyWords + 1);
                        d[u] = ((uint64_t)uni(w0.y) << 32) | uni(w0.x);
                        sr[u] = ((uint64_t)uni(w0.w) << 32) | uni(w0.z);
                        l[u] = uni(w1.x);
                    }
                }
                for (uint32_t t0 = 0; t0 < nTiles; t0 += kCopyTiles) {
                    uint32_t v[kCopyTiles][kCopyBatch];
#pragma unroll
                    for (unsigned t = 0; t < kCopyTiles; ++t) {
                        const uint32_t p = tile0 + (t0 + t) * kExecTileBytes + lane * 4;
#pragma unroll
                        for (unsigned u = 0; u < kCopyBatch; ++u)
                            v[t][u] = t0 + t < nTiles ? term_load(sr[u], l[u], p) : 0u;
                    }
#pragma unroll
                    for (unsigned t = 0; t < kCopyTiles; ++t) {
                        const uint32_t p = tile0 + (t0 + t) * kExecTileBytes + lane * 4;
                        if (t0 + t >= nTiles)
                            break;
#pragma unroll
                        for (unsigned u = 0; u < kCopyBatch; ++u) {
                            if (p < l[u])
                                st4(d[u] + p, v[t][u] & byte_mask((int)l[u] - (int)p));
                            else if (p < align16u(l[u]))
                                st4(d[u] + p, 0u);
                        }
                    }
                }
            }
        }
        if ((kind != OP_ROWS || skip) && tid < kRingWords)
            ring[cur ^ 1][tid] = pf;
        __syncthreads();
#ifdef SGPU_PHASE_CLOCKS
        if (threadIdx.x == 0 && kind >= 1 && kind <= 5) {
            atomicAdd(&g_phaseClk[32 + kind], clock64() - oclk);   // 33..37: op time by kind
            atomicAdd(&g_phaseClk[37 + kind], 1ull);               // 38..42: ops by kind
            if (kind == OP_ROWS)
                atomicAdd(&g_phaseClk[43], clock64() - t5);        // waiting for the other waves
        }
#endif
        cur ^= 1;
        pos = next;
    }
    // (the last op's barrier ordered every wave's count)
    const uint32_t tid = threadIdx.x;
    if (tid == 0 && acctL)
        atomicAdd(acct, acctL);
    PHASE_MARK(6, kclk);
    if (tid == 0) {
#ifdef SGPU_PHASE_CLOCKS
        atomicAdd(&g_phaseClk[7], 1ull);
#endif
    }
}

// ---------------------------------------------------------------------------
// Triangular solve

__device__ __forceinline__ uint32_t ld4_masked(uint64_t addr, uint32_t bytes)
{
    // first four bytes of a row, bytes at/after `bytes` read as zero
    const uint32_t v = *reinterpret_cast<const GMEM uint32_t*>(addr);
    return v & byte_mask((int)bytes);
}

// Length prefix parser (reference SiameseSerializers.h:596-627) on 4 bytes.
__device__ __forceinline__ int parse_prefix(uint32_t w, uint32_t avail, uint32_t* len)
{
    const uint32_t b0 = w & 0xff, b1 = (w >> 8) & 0xff, b2 = (w >> 16) & 0xff, b3 = w >> 24;
    if (avail < 1)
        return -1;
    const uint32_t top = b0 >> 6;
    if (top <= 1) {
        *len = b0;
        return 1;
    }
    if (top == 2) {
        if (avail < 2)
            return -1;
        *len = ((b0 << 8) | b1) & 0x3fff;
        return 2;
    }
    if ((b0 & 0xE0) == 0xC0) {
        if (avail < 3)
            return -1;
        *len = ((b0 << 16) | (b1 << 8) | b2) & 0x1fffff;
        return 3;
    }
    if (avail < 4)
        return -1;
    *len = ((b0 << 24) | (b1 << 16) | (b2 << 8) | b3) & 0x1fffffff;
    return 4;
}

// The solve's bytes 0..3 (the recovered length prefixes): MultiplyLowerTriangle
// and BackSubstitution on one dword per row (reference SiameseDecoder.cpp:
// 1065-1238) give each row's header length and length, or stop at the first
// corrupt prefix.  rw[0] = rows recovered from the right, rw[1 + i] =
// (header << 29) | length.  One wave does it with no barrier: lane l holds
// rows l, l+64, l+128, l+192 in registers (p4), row i's word reaches every
// lane by readlane, the coefficients and lengths come from the tile's LDS
// copies and per-lane multipliers from the LDS multiply tables.  Every tile
// of a solve computes the same words from the rows' first 16 bytes as copied
// before the solve (SolveDesc.head: tile 0 may already have stored solved
// rows), so the solve needs no separate launch; the tile-0 workgroup
// publishes them (`out`) with the byte counts: the diagonal scaling of
// max(32 clipped, recovered) bytes and one muladd of min(recovered, row)
// bytes per earlier row each completed step eliminates (:1131-1212).
// Ct[i*m + j] = C[j*m + i] for an m x m byte matrix, by `threads` threads
// (thread t of them), U loads in flight per thread before their stores
template <unsigned threads, unsigned U>
__device__ __forceinline__ void stage_transposed(uint8_t* __restrict__ Ct, const uint8_t* __restrict__ C,
                                                 uint32_t m, uint32_t t)
{
    const uint32_t mm = m * m;
    for (uint32_t k0 = t; k0 < mm; k0 += threads * U) {
        uint32_t v[U];
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            const uint32_t k = k0 + u * threads;
            v[u] = k < mm ? C[k] : 0u;
        }
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            const uint32_t k = k0 + u * threads;
            if (k < mm) {
                const uint32_t j = k / m, i = k - j * m;
                Ct[i * m + j] = (uint8_t)v[u];
            }
        }
    }
}

__device__ __forceinline__ uint32_t p4_get(const uint32_t (&p4)[4], uint32_t i)
{
    // row i's word (i uniform): its lane's register k = i / 64
    const uint32_t k = i >> 6;
    const uint32_t v = k == 0 ? p4[0] : k == 1 ? p4[1] : k == 2 ? p4[2] : p4[3];
    return rl(v, i & 63u);
}

#ifndef SGPU_PREFIX_PIPE
#define SGPU_PREFIX_PIPE 1
#endif
__device__ void solve_prefix_wave(uint32_t m, uint32_t lane, uint32_t (&p4)[4], const uint8_t* Ct,
                                  const uint32_t* lowL, const uint32_t* finB, const uint4* permL,
                                  const uint32_t* permC, uint32_t* rw, uint32_t* __restrict__ out,
                                  unsigned long long* __restrict__ acct)
{
#if SGPU_PREFIX_PIPE
    if (m <= 128) {
        // rows in registers 0 and 1 (lanes j = lane, lane + 64), their lower
        // lengths in registers too.  Software pipeline of depth two: during
        // step i the tables of step i+1 (from coefficients fetched during step
        // i-1) and the coefficients of step i+2 are in flight, so a step waits
        // on no LDS round trip it has not overlapped with a step's arithmetic.
        // A row with nothing to update multiplies by the zero table.
        const bool two = m > 64;
        const uint32_t j0 = lane, j1 = lane + 64, jm = m - 1;
        const uint32_t w0 = lowL[j0 < jm ? j0 : jm], w1 = lowL[j1 < jm ? j1 : jm];
        // (outside the rows a step updates, the load reads a zero byte: the
        // product table of 0, so every lane's load is unconditional)
        const uint8_t* zero = reinterpret_cast<const uint8_t*>(permL);
        auto cb = [&](uint32_t i, uint32_t j) -> uint32_t {
            return *((j > i && j < m) ? Ct + i * m + j : zero);
        };
        GfTab c0 = gf_tab_l(permL, permC, cb(0, j0)), c1 = c0;
        if (two)
            c1 = gf_tab_l(permL, permC, cb(0, j1));
        uint32_t a0 = 0, a1 = 0;
        if (m > 2) {
            a0 = cb(1, j0);
            if (two)
                a1 = cb(1, j1);
        }
        for (uint32_t i = 0; i + 1 < m; ++i) {
            const GfTab n0 = gf_tab_l(permL, permC, a0);
            GfTab n1 = c1;
            if (two)
                n1 = gf_tab_l(permL, permC, a1);
            if (i + 2 < m) {
                a0 = cb(i + 2, j0);
                if (two)
                    a1 = cb(i + 2, j1);
            }
            const uint32_t q = i & 63u;
            const bool lo = i < 64;
            const uint32_t src = rl(lo ? p4[0] : p4[1], q) & byte_mask((int)rl(lo ? w0 : w1, q));
            p4[0] ^= gf_mul_tab(src, c0);
            if (two)
                p4[1] ^= gf_mul_tab(src, c1);
            c0 = n0;
            c1 = n1;
        }
    } else
#endif
    for (uint32_t i = 0; i + 1 < m; ++i) {
        const uint32_t src = p4_get(p4, i) & byte_mask((int)uni(lowL[i]));
        const uint8_t* col = Ct + i * m;
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
            const uint32_t j = lane + 64u * k;
            if (j > i && j < m) {
                const uint32_t y = col[j];
                if (y)
                    p4[k] ^= gf_mul_tab(src, gf_tab_l(permL, permC, y));
            }
        }
    }
#ifdef SGPU_PHASE_CLOCKS
    if (lane == 0)
        atomicAdd(&g_phaseClk[48], clock64());   // the lower sweep's end (slot 45 pairs it)
#endif
    uint32_t ok = 0;
    unsigned long long opAcc = 0, outAcc = 0;
#if SGPU_PREFIX_PIPE
    if (m <= 128) {
        // back-substitution with each row's final length and diagonal-inverse
        // table in registers (lane j holds row j's) and the same two-deep
        // pipeline of update tables and coefficients as the lower sweep
        const bool two = m > 64;
        const uint32_t j0 = lane, j1 = lane + 64, jm = m - 1;
        const uint32_t r0 = j0 < jm ? j0 : jm, r1 = j1 < jm ? j1 : jm;
        const uint32_t f0 = finB[r0], f1 = finB[r1];
        const GfTab v0 = gf_tab_l(permL, permC, c_inv[Ct[r0 * m + r0]]);
        GfTab v1 = v0;
        if (two)
            v1 = gf_tab_l(permL, permC, c_inv[Ct[r1 * m + r1]]);
        const uint8_t* zero = reinterpret_cast<const uint8_t*>(permL);
        auto ub = [&](uint32_t i, uint32_t j) -> uint32_t { return *(j < i ? Ct + i * m + j : zero); };
        uint32_t y0 = ub(jm, j0), y1 = 0;
        GfTab u0 = gf_tab_l(permL, permC, y0), u1 = u0;
        if (two) {
            y1 = ub(jm, j1);
            u1 = gf_tab_l(permL, permC, y1);
        }
        uint32_t b0 = 0, b1 = 0;
        if (m >= 2) {
            b0 = ub(m - 2, j0);
            if (two)
                b1 = ub(m - 2, j1);
        }
        for (int i = (int)m - 1; i >= 0; --i) {
            const GfTab n0 = gf_tab_l(permL, permC, b0);
            GfTab n1 = u1;
            if (two)
                n1 = gf_tab_l(permL, permC, b1);
            const uint32_t z0 = b0, z1 = b1;
            if (i >= 2) {
                b0 = ub((uint32_t)i - 2, j0);
                if (two)
                    b1 = ub((uint32_t)i - 2, j1);
            }
            const uint32_t q = (uint32_t)i & 63u;
            const bool lo = i < 64;
            const uint32_t fb = rl(lo ? f0 : f1, q);
            const GfTab d{rl(lo ? v0.a0 : v1.a0, q), rl(lo ? v0.a1 : v1.a1, q), rl(lo ? v0.b0 : v1.b0, q),
                          rl(lo ? v0.b1 : v1.b1, q), rl(lo ? v0.c : v1.c, q)};
            const uint32_t lc = fb < 32 ? fb : 32;
            const uint32_t x = uni(gf_mul_tab(rl(lo ? p4[0] : p4[1], q), d)) & byte_mask((int)lc);
            uint32_t len = 0;
            const int h = parse_prefix(x, lc, &len);
            if (h < 1 || len == 0 || (uint32_t)h + len > fb)
                break;
            const uint32_t b = (uint32_t)h + len;
            if (lane == 0) {
                rw[1 + i] = ((uint32_t)h << 29) | len;
                opAcc += lc > b ? lc : b;
                outAcc += b;
            }
            ++ok;
            const uint32_t xi = x & byte_mask((int)b);
            if (y0) {
                const uint32_t ab = b < f0 ? b : f0;
                p4[0] ^= gf_mul_tab(xi & byte_mask((int)ab), u0);
                opAcc += ab;
            }
            if (two && y1) {
                const uint32_t ab = b < f1 ? b : f1;
                p4[1] ^= gf_mul_tab(xi & byte_mask((int)ab), u1);
                opAcc += ab;
            }
            u0 = n0;
            u1 = n1;
            y0 = z0;
            y1 = z1;
        }
    } else
#endif
    for (int i = (int)m - 1; i >= 0; --i) {
        const uint8_t* col = Ct + (uint32_t)i * m;
        const uint32_t fb = uni(finB[i]);
        const uint32_t lc = fb < 32 ? fb : 32;
        const uint32_t x = gf_mul_dword(p4_get(p4, (uint32_t)i), inv_u(uni(col[i]))) & byte_mask((int)lc);
        uint32_t len = 0;
        const int h = parse_prefix(x, lc, &len);
        if (h < 1 || len == 0 || (uint32_t)h + len > fb)
            break;
        const uint32_t b = (uint32_t)h + len;
        if (lane == 0) {
            rw[1 + i] = ((uint32_t)h << 29) | len;
            opAcc += lc > b ? lc : b;
            outAcc += b;
        }
        ++ok;
        const uint32_t xi = x & byte_mask((int)b);
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
            const uint32_t j = lane + 64u * k;
            if (j < (uint32_t)i) {
                const uint32_t c = col[j];
                if (c) {
                    const uint32_t fj = finB[j];
                    const uint32_t ab = b < fj ? b : fj;
                    p4[k] ^= gf_mul_tab(xi & byte_mask((int)ab), gf_tab_l(permL, permC, c));
                    opAcc += ab;
                }
            }
        }
    }
    if (lane == 0)
        rw[0] = ok;
    for (uint32_t j = lane; j + ok < m; j += 64)
        rw[1 + j] = 0;   // rows not reached (the host does not read them)
    if (out) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t k = lane; k <= m; k += 64)
            out[k] = rw[k];
        // the product solves' tail flag: clear on every path (k_solve_tr, which
        // runs after this pass where it runs at all, sets it), so that the host
        // reads it of every completed solve (sgpu_engine_stats_ex [40])
        if (lane == 0)
            out[m + 1] = 0;
        // one atomic per wave (per-lane global atomics serialise at one address)
#pragma unroll
        for (unsigned d = 32; d >= 1; d >>= 1) {
            opAcc += __shfl_xor(opAcc, d, 64);
            outAcc += __shfl_xor(outAcc, d, 64);
        }
        if (lane == 0 && opAcc)
            atomicAdd(&acct[0], opAcc);
        if (lane == 0 && outAcc)
            atomicAdd(&acct[1], outAcc);
    }
}

// A solve gated on a chained device elimination that failed (SolveDesc.gate):
// its coefficients and row order were never written, so it does not run.
__device__ __forceinline__ bool solve_gated_off(const SolveDesc& sd, const uint32_t* results)
{
    return sd.gate != 0 && results[sd.gate - 1u] == 0u;
}

// rows' first words for the prefix pass (wave 0), loaded before the staging
// so their latency overlaps it
__device__ __forceinline__ void prefix_load(uint32_t (&p4)[4], uint32_t m, uint32_t lane, uint64_t head,
                                            const SolveRow* __restrict__ R)
{
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        const uint32_t j = lane + 64u * k;
        p4[k] = j < m ? ld4_masked(head + (uint64_t)solve_head_slot(R[j].headIndex, j) * 16u, R[j].initBytes) : 0u;
    }
}

// k_solve_main: one workgroup of kSolveWaves waves per (solve, tile).  Wave 0
// first solves the length prefixes (solve_prefix_wave) while the others wait.
//
// 1 KiB tiles (m <= kSolveWideMaxRows): the tile of all m rows is staged in
// LDS once (bytes past each row's initial length read as zero:
// the reference's zero-padded growth), wave w owns rows j = w (mod W), and
// both triangular sweeps run in LDS with one barrier per pivot step.  Each
// recovered row is stored once, right after its back-substitution step;
// rows left unsolved (a corrupt length prefix) are stored at the end.  HBM
// traffic is one read and one write of each row instead of ~m of each.
//
// 256-byte tiles (m > kSolveWideMaxRows): the same sweeps (solve_tile_narrow
// below), up to the 255-column limit.  Both need ~140 KiB of dynamic LDS at
// their largest m, which gfx950 grants (be_init fails otherwise).
//
// The staged rows take m KiB of LDS, so only one or two workgroups fit on a
// CU.  Eight waves per workgroup measured best (A/B of 4/8/16: 16 waves put
// more waves on each pivot step's barrier than its few row updates use).
#ifndef SGPU_SOLVE_WAVES
#define SGPU_SOLVE_WAVES 8
#endif
constexpr unsigned kSolveWaves = SGPU_SOLVE_WAVES;
constexpr unsigned kSolveLdsMaxRows = 255;   // kMaximumLossRecoveryCount (SiameseCommon.h:80)

// LDS bytes of the staged solve: row tiles, the transposed coefficient
// matrix, per-row lengths and the result words.
// (the multiply tables at the end only when the tiles run the prefix pass:
// 5 KiB more can halve the workgroups that fit a CU)
__host__ __device__ constexpr uint32_t solve_lds_bytes(uint32_t m, bool prefix = true)
{
    return m * 1024u + ((m * m + 15u) & ~15u) + ((m * 12u + (m + 1u) * 4u + 15u) & ~15u) +
           (prefix ? 256u * 20u : 0u);
}

__device__ void solve_tile_lds(uint4* __restrict__ X, uint32_t m, const SolveRow* __restrict__ R,
                               const uint8_t* __restrict__ C, uint64_t head, const uint32_t* __restrict__ resIn,
                               uint32_t* __restrict__ out, unsigned long long* __restrict__ acct,
                               uint32_t tileBase)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    const uint32_t wave = tid >> 6;
    const uint32_t p = tileBase + lane * 16;
    // Everything the sweeps consult goes to LDS first, so no step of the
    // serial pivot chain waits on a global-memory round trip.
    uint8_t* Ct = reinterpret_cast<uint8_t*>(X + m * 64);        // Ct[i*m + j] = C[j][i]
    uint32_t* initB = reinterpret_cast<uint32_t*>(Ct + ((m * m + 15u) & ~15u));
    uint32_t* lowL = initB + m;
    uint32_t* finB = lowL + m;
    uint32_t* rw = finB + m;                                     // result words
    uint4* permL = reinterpret_cast<uint4*>(initB + ((m * 12u + (m + 1u) * 4u + 15u) & ~15u) / 4u);
    uint32_t* permC = reinterpret_cast<uint32_t*>(permL + 256);  // (prefix pass only)

    uint32_t p4[4];
    if (resIn) {
        for (uint32_t k = tid; k <= m; k += 64 * kSolveWaves)
            rw[k] = resIn[k];   // (solved by k_solve_prefix)
    } else {
        if (wave == 0)
            prefix_load(p4, m, lane, head, R);
        for (uint32_t y = tid; y < 256; y += 64 * kSolveWaves) {
            const uint32_t* t = c_perm[y];
            permL[y] = make_uint4(t[0], t[1], t[2], t[3]);
            permC[y] = t[4];
        }
    }
    stage_transposed<64 * kSolveWaves, 4>(Ct, C, m, tid);
    for (uint32_t j = tid; j < m; j += 64 * kSolveWaves) {
        initB[j] = R[j].initBytes;
        lowL[j] = R[j].lowerLen;
        finB[j] = R[j].finalBytes;
    }
    // row tiles: wave w stages rows w, w+W, ... four loads in flight per lane
    for (uint32_t j0 = wave; j0 < m; j0 += 4 * kSolveWaves) {
        uint4 v[4];
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) {
            const uint32_t j = j0 + u * kSolveWaves;
            v[u] = make_uint4(0, 0, 0, 0);
            if (j < m) {
                const uint32_t ib = R[j].initBytes;
                if (p < ib) {
                    v[u] = ld16(R[j].buf + p);
                    if (p + 16 > ib)
                        v[u] = mask16(v[u], (int)ib - (int)p);
                }
            }
        }
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) {
            const uint32_t j = j0 + u * kSolveWaves;
            if (j < m)
                X[j * 64 + lane] = v[u];
        }
    }
    __syncthreads();
    if (!resIn) {
        if (wave == 0)
            solve_prefix_wave(m, lane, p4, Ct, lowL, finB, permL, permC, rw, out, acct);
        __syncthreads();
    }

    // MultiplyLowerTriangle in pivot order (reference SiameseDecoder.cpp:1065-1104)
    // LDS values read by every lane alike are moved to scalar registers
    // (uni), so the GF multiplier tables are fetched with scalar loads and
    // the branches around the barriers are visibly uniform.
    for (uint32_t i = 0; i + 1 < m; ++i) {
        const uint32_t L = uni(lowL[i]);
        if (tileBase >= L)
            continue;   // uniform: row i contributes nothing to this tile
        uint4 src = X[i * 64 + lane];
        if (p + 16 > L)
            src = mask16(src, (int)L - (int)p);
        const uint8_t* col = Ct + i * m;
        const Split16 ss = gf_split16(src);
        const uint32_t first = i + 1 + ((wave + kSolveWaves - (i + 1) % kSolveWaves) % kSolveWaves);
        // four independent row updates at a time, so the coefficient and
        // table fetches of one overlap those of the others
        for (uint32_t j0 = first; j0 < m; j0 += 4 * kSolveWaves) {
            uint32_t y[4];
            uint4 xr[4];
#pragma unroll
            for (unsigned u = 0; u < 4; ++u) {
                const uint32_t j = j0 + u * kSolveWaves;
                y[u] = j < m ? uni(col[j]) : 0;
                xr[u] = j < m ? X[j * 64 + lane] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (unsigned u = 0; u < 4; ++u) {
                const uint32_t j = j0 + u * kSolveWaves;
                if (y[u])
                    X[j * 64 + lane] = xor16(xr[u], gf_mul16_split(ss, gf_tab(y[u])));
            }
        }
        __syncthreads();
    }

    // BackSubstitution from the right-most column (reference :1106-1238)
    const uint32_t ok = uni(rw[0]);
    uint32_t done = 0;
    for (int i = (int)m - 1; i >= 0 && done < ok; --i, ++done) {
        const uint32_t w = uni(rw[1 + i]);
        const uint32_t bb = (w >> 29) + (w & kSolveLengthMask);
        const uint8_t* col = Ct + (uint32_t)i * m;
        uint4 x = gf_mul16(X[i * 64 + lane], inv_u(uni(col[i])));
        x = mask16(x, (int)bb - (int)p); // zero beyond the recovered length
        if ((uint32_t)i % kSolveWaves == wave && p < finB[i])
            st16(R[i].buf + p, x);
        if (tileBase < bb) {
            const Split16 xsp = gf_split16(x);
            for (uint32_t j0 = wave; j0 < (uint32_t)i; j0 += 4 * kSolveWaves) {
                uint32_t c[4], fj[4];
                uint4 xr[4];
#pragma unroll
                for (unsigned u = 0; u < 4; ++u) {
                    const uint32_t j = j0 + u * kSolveWaves;
                    c[u] = j < (uint32_t)i ? uni(col[j]) : 0;
                    fj[u] = j < (uint32_t)i ? uni(finB[j]) : 0;
                    xr[u] = j < (uint32_t)i ? X[j * 64 + lane] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (unsigned u = 0; u < 4; ++u) {
                    if (!c[u])
                        continue;
                    const uint32_t j = j0 + u * kSolveWaves;
                    const uint32_t ab = bb < fj[u] ? bb : fj[u];
                    // (multiply, then clip: GF(256) products keep zero bytes zero)
                    uint4 prod = gf_mul16_split(xsp, gf_tab(c[u]));
                    if (ab < tileBase + kTileBytes)
                        prod = mask16(prod, (int)ab - (int)p);
                    X[j * 64 + lane] = xor16(xr[u], prod);
                }
            }
        }
        __syncthreads();
    }
    // rows the back-substitution did not reach
    for (uint32_t j = wave; j + done < m; j += kSolveWaves)
        if (p < finB[j])
            st16(R[j].buf + p, X[j * 64 + lane]);
}

// Narrow LDS path (kSolveWideMaxRows < m <= 255): 256-byte tiles, so the m
// row tiles (<= 64 KiB) and the m x m coefficients (<= 64 KiB) fit one
// workgroup's LDS together.  A row tile is 16 lanes x 16 bytes: lane = 16 q
// + c holds chunk c of one of four rows per wave (row slot 4 w + q, 32 slots
// per workgroup), so each row update's multiplier differs per quad and comes
// from the workgroup's LDS copy of the multiply tables.  Same sweeps, same
// barriers and same stores as the 1 KiB path.
__host__ __device__ constexpr uint32_t solve_narrow_lds_bytes(uint32_t m)
{
    return m * kSolveNarrowTileBytes + ((m * m + 15u) & ~15u) + 256u * 20u + m * 12u + (m + 1u) * 4u;
}

__device__ void solve_tile_narrow(uint4* __restrict__ X, uint32_t m, const SolveRow* __restrict__ R,
                                  const uint8_t* __restrict__ C, uint64_t head, const uint32_t* __restrict__ resIn,
                                  uint32_t* __restrict__ out, unsigned long long* __restrict__ acct,
                                  uint32_t tileBase)
{
    constexpr uint32_t kChunks = kSolveNarrowTileBytes / 16;   // 16 lanes per row
    constexpr uint32_t kSlots = kSolveWaves * (64 / kChunks);  // rows in flight per workgroup
    const uint32_t tid = threadIdx.x;
    const uint32_t c = tid & (kChunks - 1);
    const uint32_t slot = tid / kChunks;
    const uint32_t p = tileBase + c * 16;
    uint4* permL = X + m * kChunks;                                  // c_perm words 0..3
    uint32_t* permC = reinterpret_cast<uint32_t*>(permL + 256);      // c_perm word 4
    uint8_t* Ct = reinterpret_cast<uint8_t*>(permC + 256);           // Ct[i*m + j] = C[j][i]
    uint32_t* initB = reinterpret_cast<uint32_t*>(Ct + ((m * m + 15u) & ~15u));
    uint32_t* lowL = initB + m;
    uint32_t* finB = lowL + m;
    uint32_t* rw = finB + m;

    uint32_t p4[4];
    if (resIn) {
        for (uint32_t k = tid; k <= m; k += 64 * kSolveWaves)
            rw[k] = resIn[k];   // (solved by k_solve_prefix)
    } else if (tid < 64) {
        prefix_load(p4, m, tid, head, R);
    }
    for (uint32_t y = tid; y < 256; y += 64 * kSolveWaves) {
        const uint32_t* t = c_perm[y];
        permL[y] = make_uint4(t[0], t[1], t[2], t[3]);
        permC[y] = t[4];
    }
    stage_transposed<64 * kSolveWaves, 4>(Ct, C, m, tid);
    for (uint32_t j = tid; j < m; j += 64 * kSolveWaves) {
        initB[j] = R[j].initBytes;
        lowL[j] = R[j].lowerLen;
        finB[j] = R[j].finalBytes;
    }
    // row tiles, bytes past each row's initial length as zero; four loads
    // in flight per lane
    for (uint32_t j0 = slot; j0 < m; j0 += 4 * kSlots) {
        uint4 v[4];
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) {
            const uint32_t j = j0 + u * kSlots;
            v[u] = make_uint4(0, 0, 0, 0);
            if (j < m) {
                const uint32_t ib = R[j].initBytes;
                if (p < ib) {
                    v[u] = ld16(R[j].buf + p);
                    if (p + 16 > ib)
                        v[u] = mask16(v[u], (int)ib - (int)p);
                }
            }
        }
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) {
            const uint32_t j = j0 + u * kSlots;
            if (j < m)
                X[j * kChunks + c] = v[u];
        }
    }
    __syncthreads();
    if (!resIn) {
        if (tid < 64)
            solve_prefix_wave(m, tid, p4, Ct, lowL, finB, permL, permC, rw, out, acct);
        __syncthreads();
    }

    // MultiplyLowerTriangle in pivot order (reference SiameseDecoder.cpp:1065-1104)
    for (uint32_t i = 0; i + 1 < m; ++i) {
        const uint32_t L = uni(lowL[i]);
        if (tileBase >= L)
            continue;   // uniform: row i contributes nothing to this tile
        uint4 src = X[i * kChunks + c];
        if (p + 16 > L)
            src = mask16(src, (int)L - (int)p);
        const uint8_t* col = Ct + i * m;
        const uint32_t first = i + 1 + ((slot + kSlots - (i + 1) % kSlots) % kSlots);
        for (uint32_t j0 = first; j0 < m; j0 += 2 * kSlots) {
            uint32_t y[2];
            uint4 xr[2];
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint32_t j = j0 + u * kSlots;
                y[u] = j < m ? col[j] : 0;
                xr[u] = j < m ? X[j * kChunks + c] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint32_t j = j0 + u * kSlots;
                if (y[u])
                    X[j * kChunks + c] = xor16(xr[u], gf_mul16_tab(src, gf_tab_l(permL, permC, y[u])));
            }
        }
        __syncthreads();
    }

    // BackSubstitution from the right-most column (reference :1106-1238)
    const uint32_t ok = uni(rw[0]);
    uint32_t done = 0;
    for (int i = (int)m - 1; i >= 0 && done < ok; --i, ++done) {
        const uint32_t w = uni(rw[1 + i]);
        const uint32_t bb = (w >> 29) + (w & kSolveLengthMask);
        const uint8_t* col = Ct + (uint32_t)i * m;
        uint4 x = gf_mul16(X[i * kChunks + c], inv_u(uni(col[i])));
        x = mask16(x, (int)bb - (int)p); // zero beyond the recovered length
        if (slot == (uint32_t)i % kSlots && p < finB[i])
            st16(R[i].buf + p, x);
        if (tileBase < bb) {
            for (uint32_t j0 = slot; j0 < (uint32_t)i; j0 += 2 * kSlots) {
                uint32_t cj[2], fj[2];
                uint4 xr[2];
#pragma unroll
                for (unsigned u = 0; u < 2; ++u) {
                    const uint32_t j = j0 + u * kSlots;
                    cj[u] = j < (uint32_t)i ? col[j] : 0;
                    fj[u] = j < (uint32_t)i ? finB[j] : 0;
                    xr[u] = j < (uint32_t)i ? X[j * kChunks + c] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (unsigned u = 0; u < 2; ++u) {
                    if (!cj[u])
                        continue;
                    const uint32_t j = j0 + u * kSlots;
                    const uint32_t ab = bb < fj[u] ? bb : fj[u];
                    const uint4 xs = mask16(x, (int)ab - (int)p);
                    X[j * kChunks + c] = xor16(xr[u], gf_mul16_tab(xs, gf_tab_l(permL, permC, cj[u])));
                }
            }
        }
        __syncthreads();
    }
    // rows the back-substitution did not reach
    for (uint32_t j = slot; j + done < m; j += kSlots)
        if (p < finB[j])
            st16(R[j].buf + p, X[j * kChunks + c]);
}

// bytes of dynamic LDS a solve launch needs for its largest m
__host__ __device__ constexpr uint32_t solve_launch_lds_bytes(uint32_t maxRows, bool prefix = true)
{
    return maxRows > kSolveWideMaxRows
               ? (solve_narrow_lds_bytes(maxRows) > solve_lds_bytes(kSolveWideMaxRows, prefix)
                      ? solve_narrow_lds_bytes(maxRows)
                      : solve_lds_bytes(kSolveWideMaxRows, prefix))
               : solve_lds_bytes(maxRows, prefix);
}

__global__ __launch_bounds__(64 * kSolveWaves) void k_solve_main(
    const SolveDesc* __restrict__ solves, const SolveRow* __restrict__ rows,
    const uint8_t* __restrict__ coef, uint32_t* __restrict__ results,
    const SolveItem* __restrict__ items, unsigned long long* __restrict__ acct, uint32_t flags)
{
    extern __shared__ uint4 X[];
    const SolveItem it = items[blockIdx.x];
    const SolveDesc sd = solves[it.solve];
    const uint32_t m = sd.m;
    const SolveRow* R = rows + sd.rowBegin;
    const uint8_t* C = coef + sd.coefOffset;
    if (m > kSolveLdsMaxRows || solve_gated_off(sd, results))
        return;   // (the host never queues m > 255: kMaximumLossRecoveryCount)
    // flags bit 0: the length prefixes are already solved (k_solve_prefix or
    // k_solve_pre); bit 2: k_solve_tr ran before this launch (it took every
    // solve it could, into the scratch)
    const bool prefixDone = (flags & 1u) != 0;
    if ((flags & 6u) && m <= kProductMaxRows && sd.tinv && results[sd.result] == m &&
        results[sd.result + m + 1] == 0) {
        // solved as X = T R (k_solve_tr), every row zero past
        // its recovered length, so the sweeps' clipping would change nothing:
        // this tile of the result rows from the scratch into the rows (bytes
        // below each row's final length).  A solve whose products have
        // non-zero bytes there (inconsistent recovery data) falls through to
        // the sweeps, on its rows as they were: the products went to scratch.
        static_assert(kProductMaxRows <= kSolveWideMaxRows, "product solves take 1 KiB tiles");
        const uint32_t xs = solve_x_stride(sd.maxBytes), tb = kTileBytes;
        for (uint32_t x = threadIdx.x; x < m * (tb / 16u); x += 64u * kSolveWaves) {
            const uint32_t i = x / (tb / 16u), p = it.tileBase + 16u * (x - i * (tb / 16u));
            if (p < R[i].finalBytes)
                st16(R[i].buf + p, ld16(sd.xout + (uint64_t)i * xs + p));
        }
        return;
    }
    const uint32_t* resIn = prefixDone ? results + sd.result : nullptr;
    uint32_t* out = (!prefixDone && it.tileBase == 0) ? results + sd.result : nullptr;
    if (m <= kSolveWideMaxRows)
        solve_tile_lds(X, m, R, C, sd.head, resIn, out, acct, it.tileBase);
    else
        solve_tile_narrow(X, m, R, C, sd.head, resIn, out, acct, it.tileBase);
}

// k_solve_prefix: the length-prefix pass alone, one wave per solve, ahead of
// k_solve_main when a launch holds many solves (the fused pass would run on
// every tile of every solve, serially before its sweeps).
__host__ __device__ constexpr uint32_t solve_prefix_lds_bytes(uint32_t m)
{
    return 256u * 20u + ((m * m + 15u) & ~15u) + m * 8u + (m + 1u) * 4u;
}

__global__ __launch_bounds__(64) void k_solve_prefix(const SolveDesc* __restrict__ solves,
                                                     const SolveRow* __restrict__ rows,
                                                     const uint8_t* __restrict__ coef,
                                                     uint32_t* __restrict__ results,
                                                     unsigned long long* __restrict__ acct)
{
    extern __shared__ uint4 X[];
    const SolveDesc sd = solves[blockIdx.x];
    const uint32_t m = sd.m;
    if (m > kSolveLdsMaxRows || solve_gated_off(sd, results))
        return;
    const SolveRow* R = rows + sd.rowBegin;
    const uint8_t* C = coef + sd.coefOffset;
    const uint32_t lane = threadIdx.x;
    uint4* permL = X;
    uint32_t* permC = reinterpret_cast<uint32_t*>(permL + 256);
    uint8_t* Ct = reinterpret_cast<uint8_t*>(permC + 256);
    uint32_t* lowL = reinterpret_cast<uint32_t*>(Ct + ((m * m + 15u) & ~15u));
    uint32_t* finB = lowL + m;
    uint32_t* rw = finB + m;
    uint32_t p4[4];
#ifdef SGPU_PHASE_CLOCKS
    const unsigned long long pclk = clock64();
#endif
    prefix_load(p4, m, lane, sd.head, R);
    for (uint32_t y = lane; y < 256; y += 64) {
        const uint32_t* t = c_perm[y];
        permL[y] = make_uint4(t[0], t[1], t[2], t[3]);
        permC[y] = t[4];
    }
    // the coefficients, transposed: eight loads in flight per lane (one wave
    // stages up to 255^2 bytes; a load-then-store loop would pay a memory
    // round trip per 64 bytes)
    stage_transposed<64, 8>(Ct, C, m, lane);
    for (uint32_t j = lane; j < m; j += 64) {
        lowL[j] = R[j].lowerLen;
        finB[j] = R[j].finalBytes;
    }
    __syncthreads();
#ifdef SGPU_PHASE_CLOCKS
    // slots 44-47: setup clocks, solve clocks, sum of m, the largest solve's clocks
    const unsigned long long sclk = clock64();
    if (lane == 0) {
        atomicAdd(&g_phaseClk[44], sclk - pclk);
        atomicAdd(&g_phaseClk[46], (unsigned long long)m);
        atomicAdd(&g_phaseClk[49], sclk);
    }
#endif
    solve_prefix_wave(m, lane, p4, Ct, lowL, finB, permL, permC, rw, results + sd.result, acct);
#ifdef SGPU_PHASE_CLOCKS
    if (lane == 0) {
        const unsigned long long e = clock64();
        atomicAdd(&g_phaseClk[45], e - sclk);
        atomicMax(&g_phaseClk[47], (e - pclk) << 8 | (m & 0xffu));
    }
#endif
}

// ---------------------------------------------------------------------------
// The product solve's inverse and length prefixes (k_solve_pre)
//
// The solve's result rows are X = T R, with T = U^-1 L^-1 the m x m inverse
// of the eliminated coefficient matrix (MultiplyLowerTriangle applies L^-1,
// BackSubstitution U^-1; reference SiameseDecoder.cpp:1065-1238); k_solve_tr
// forms the product.
//
// k_solve_pre (one launch, two kinds of workgroup):
//   workgroups [0, n): the length-prefix pass of solve b (all waves stage the
//   coefficients, then wave 0 runs solve_prefix_wave);
//   workgroups [n, 2n): T of solve b - n, the reference's two sweeps applied
//   to the identity in LDS (rows of m <= 120 bytes, one half-wave a row),
//   written to the solve's scratch (SolveDesc.tinv, rows of kTStride bytes).
// The two kinds run side by side, so T costs no time on the prefix pass's
// serial critical path.  The product runs only when the prefix pass found
// every recovered length valid (results[0] == m): the exact sweeps and the
// prefixes then agree byte for byte, since bytes past a row's length are zero
// in the true originals.  A solve with a corrupt prefix, or m >
// kProductMaxRows, is left to k_solve_main, which reproduces the reference's
// partial back-substitution exactly.  (The same product on the int8 matrix
// cores was built and measured slower: tools/variants/solve_mfma.hip.)
constexpr unsigned kPreWaves = 8;
constexpr unsigned kPreThreads = 64 * kPreWaves;

__host__ __device__ constexpr uint32_t t_rows(uint32_t m) { return (m + 3u) & ~3u; }
// k_solve_pre: the larger of the prefix pass's staging and the T build's
__host__ __device__ constexpr uint32_t solve_tbuild_lds_bytes(uint32_t m)
{
    return ((m * m + 15u) & ~15u) + t_rows(m) * kTStride + 256u * 20u + 256u;
}
__host__ __device__ constexpr uint32_t solve_pre_lds_bytes(uint32_t m)
{
    return solve_prefix_lds_bytes(m) > solve_tbuild_lds_bytes(m < kProductMaxRows ? m : kProductMaxRows)
               ? solve_prefix_lds_bytes(m)
               : solve_tbuild_lds_bytes(m < kProductMaxRows ? m : kProductMaxRows);
}

// One T-build step's row updates: rows j in [j0, j1) (this half-wave's,
// stride kPreThreads / 32) take Y_j ^= Ct[c0 + j] a ^ Ct[c1 + j] b.  Four
// rows at a time with every LDS read of the four issued before any product,
// and the two sources' multiply fields split once: the rows' chains overlap
// instead of running one LDS round trip after another.
__device__ __forceinline__ void tbuild_rows(uint32_t* Yw, const uint8_t* Ct, const uint4* permL, const uint32_t* permC,
                                            uint32_t m, uint32_t j0, uint32_t j1, uint32_t hw, uint32_t l32,
                                            uint32_t c0, uint32_t c1, uint32_t a, uint32_t b)
{
    constexpr uint32_t kHalves = kPreThreads / 32;
    const uint32_t aa = a & 0x07070707u, ab = (a >> 3) & 0x07070707u, ac = (a >> 6) & 0x03030303u;
    const uint32_t ba = b & 0x07070707u, bb = (b >> 3) & 0x07070707u, bc = (b >> 6) & 0x03030303u;
    for (uint32_t j = j0 + hw; j < j1; j += 4 * kHalves) {
        uint32_t cur[4];
        GfTab t0[4], t1[4];
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) {
            const uint32_t r = j + u * kHalves;
            const bool in = r < j1;
            const uint32_t y0 = in ? Ct[c0 + r] : 0u, y1 = in ? Ct[c1 + r] : 0u;
            t0[u] = gf_tab_l(permL, permC, y0);   // (the table of 0 gives 0)
            t1[u] = gf_tab_l(permL, permC, y1);
            cur[u] = in ? Yw[r * 32 + l32] : 0u;
        }
#pragma unroll
        for (unsigned u = 0; u < 4; ++u) {
            const uint32_t r = j + u * kHalves;
            if (r < j1)
                Yw[r * 32 + l32] = __builtin_amdgcn_bitop3_b32(
                    cur[u],
                    __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(t0[u].a1, t0[u].a0, aa),
                                                __builtin_amdgcn_perm(t0[u].b1, t0[u].b0, ab),
                                                __builtin_amdgcn_perm(0u, t0[u].c, ac), 0x96),
                    __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(t1[u].a1, t1[u].a0, ba),
                                                __builtin_amdgcn_perm(t1[u].b1, t1[u].b0, bb),
                                                __builtin_amdgcn_perm(0u, t1[u].c, bc), 0x96),
                    0x96);
        }
    }
}

// T = U^-1 L^-1 of solve sd into sd.tinv (all waves of the workgroup)
__device__ void solve_tbuild(const SolveDesc& sd, const uint8_t* __restrict__ C, uint8_t* base, uint32_t tid)
{
    const uint32_t m = sd.m, mp = t_rows(m);
    uint8_t* Ct = base;                                          // Ct[i*m + j] = C[j][i]
    uint8_t* Y = Ct + ((m * m + 15u) & ~15u);                    // T, rows of kTStride bytes
    uint4* permL = reinterpret_cast<uint4*>(Y + mp * kTStride);
    uint32_t* permC = reinterpret_cast<uint32_t*>(permL + 256);
    // the diagonal's inverses from LDS: c_inv indexed by a value read from
    // LDS is a memory round trip on the back-substitution's serial chain
    uint8_t* invB = reinterpret_cast<uint8_t*>(permC + 256);
    stage_transposed<kPreThreads, 2>(Ct, C, m, tid);
    if (tid < 64)
        reinterpret_cast<uint32_t*>(invB)[tid] = reinterpret_cast<const uint32_t*>(c_inv)[tid];
    if (tid < 256) {
        const uint32_t* t = c_perm[tid];
        permL[tid] = make_uint4(t[0], t[1], t[2], t[3]);
        permC[tid] = t[4];
    }
    // T starts as the identity (rows past m stay zero)
    uint32_t* Yw = reinterpret_cast<uint32_t*>(Y);
    for (uint32_t k = tid; k < mp * (kTStride / 4); k += kPreThreads) {
        const uint32_t i = k / (kTStride / 4), c4 = (k % (kTStride / 4)) * 4;
        Yw[k] = (i < m && i >= c4 && i < c4 + 4) ? 1u << (8 * (i - c4)) : 0u;
    }
    __syncthreads();
    // MultiplyLowerTriangle, then BackSubstitution, on the identity's rows (a
    // row of T is m <= 120 bytes: one half-wave, four bytes a lane), two
    // pivots per barrier: every half-wave forms the second pivot's row from
    // the first itself, so a step applies both to the rows past them (two
    // multiplies a row) and the serial chain is m barriers instead of 2m.
    // The second pivot's new row is written after the step's barrier (no
    // later step of the sweep reads it; the other half-waves read the old one
    // during the step).
    constexpr uint32_t kHalves = kPreThreads / 32;
    const uint32_t hw = tid >> 5, l32 = tid & 31;
    auto mul = [&](uint32_t v, uint32_t y) { return y ? gf_mul_tab(v, gf_tab_l(permL, permC, y)) : 0u; };
    uint32_t pend = 0, pendRow = 0xffffffffu;   // a pivot row to store (half-wave 0)
    auto flush_pend = [&]() {
        if (pendRow != 0xffffffffu && hw == 0)
            Yw[pendRow * 32 + l32] = pend;
        pendRow = 0xffffffffu;
    };
    {
        uint32_t i = 0;
        for (; i + 2 < m; i += 2) {
            flush_pend();
            const uint32_t a = Yw[i * 32 + l32];
            const uint32_t b = Yw[(i + 1) * 32 + l32] ^ mul(a, Ct[i * m + i + 1]);   // row i+1 after pivot i
            tbuild_rows(Yw, Ct, permL, permC, m, i + 2, m, hw, l32, i * m, (i + 1) * m, a, b);
            pend = b;
            pendRow = i + 1;
            __syncthreads();
        }
        flush_pend();
        if (i + 1 < m) {
            // (one pivot left before the last row)
            const uint32_t src = Yw[i * 32 + l32];
            for (uint32_t j = i + 1 + hw; j < m; j += kHalves) {
                const uint32_t y = Ct[i * m + j];
                if (y)
                    Yw[j * 32 + l32] ^= mul(src, y);
            }
        }
        __syncthreads();
    }
    {
        int i = (int)m - 1;
        for (; i >= 2; i -= 2) {
            flush_pend();
            const uint32_t xi = mul(Yw[i * 32 + l32], invB[Ct[i * m + i]]);
            const uint32_t ym = Yw[(i - 1) * 32 + l32] ^ mul(xi, Ct[(uint32_t)i * m + i - 1]);   // row i-1 after pivot i
            const uint32_t xm = mul(ym, invB[Ct[(i - 1) * m + i - 1]]);
            tbuild_rows(Yw, Ct, permL, permC, m, 0, (uint32_t)i - 1, hw, l32, (uint32_t)i * m, (uint32_t)(i - 1) * m, xi,
                        xm);
            pend = ym;
            pendRow = (uint32_t)i - 1;
            __syncthreads();
        }
        flush_pend();
        if (i == 1) {
            const uint32_t xi = mul(Yw[32 + l32], invB[Ct[m + 1]]);
            if (hw == 0) {
                const uint32_t y = Ct[m];   // C[0][1]
                if (y)
                    Yw[l32] ^= mul(xi, y);
            }
        }
        __syncthreads();
    }
    GMEM uint32_t* out = reinterpret_cast<GMEM uint32_t*>(sd.tinv);
    for (uint32_t k = tid; k < mp * 32u; k += kPreThreads) {
        const uint32_t i = k >> 5;
        out[k] = i < m ? gf_mul_tab(Yw[k], gf_tab_l(permL, permC, invB[Ct[i * m + i]])) : 0u;
    }
}

__global__ __launch_bounds__(kPreThreads) void k_solve_pre(const SolveDesc* __restrict__ solves,
                                                          const SolveRow* __restrict__ rows,
                                                          const uint8_t* __restrict__ coef,
                                                          uint32_t* __restrict__ results,
                                                          unsigned long long* __restrict__ acct,
                                                          uint32_t count, uint32_t mode)
{
    // mode 0: workgroups [0, count) prefix passes, [count, 2 count) inverses;
    // 1: inverses only (workgroup b: solve b); 2: prefix passes only
    extern __shared__ uint4 X[];
    const uint32_t tid = threadIdx.x;
    if (mode == 1 || (mode == 0 && blockIdx.x >= count)) {
        const SolveDesc sd = solves[mode == 1 ? blockIdx.x : blockIdx.x - count];
        if (sd.m == 0 || sd.m > kProductMaxRows || sd.tinv == 0 || solve_gated_off(sd, results))
            return;   // (uniform)
        solve_tbuild(sd, coef + sd.coefOffset, reinterpret_cast<uint8_t*>(X), tid);
        return;
    }
    const SolveDesc sd = solves[blockIdx.x];
    const uint32_t m = sd.m;
    if (m > kSolveLdsMaxRows || solve_gated_off(sd, results))
        return;
    const SolveRow* R = rows + sd.rowBegin;
    const uint8_t* C = coef + sd.coefOffset;
    uint4* permL = X;
    uint32_t* permC = reinterpret_cast<uint32_t*>(permL + 256);
    uint8_t* Ct = reinterpret_cast<uint8_t*>(permC + 256);
    uint32_t* lowL = reinterpret_cast<uint32_t*>(Ct + ((m * m + 15u) & ~15u));
    uint32_t* finB = lowL + m;
    uint32_t* rw = finB + m;
    uint32_t p4[4];
    if (tid < 64)
        prefix_load(p4, m, tid, sd.head, R);
    if (tid < 256) {
        const uint32_t* t = c_perm[tid];
        permL[tid] = make_uint4(t[0], t[1], t[2], t[3]);
        permC[tid] = t[4];
    }
    if (tid == 0)
        results[sd.result + m + 1] = 0;   // the product solves' tail flag
    // (every wave stages; then wave 0 alone runs the serial pass)
    stage_transposed<kPreThreads, 2>(Ct, C, m, tid);
    for (uint32_t j = tid; j < m; j += kPreThreads) {
        lowL[j] = R[j].lowerLen;
        finB[j] = R[j].finalBytes;
    }
    __syncthreads();
    if (tid >= 64)
        return;
    solve_prefix_wave(m, tid, p4, Ct, lowL, finB, permL, permC, rw, results + sd.result, acct);
}

// ---------------------------------------------------------------------------
// The same product on the vector ALUs (k_solve_tr; the default for launches
// of many solves)
//
// X = T R for the solves k_solve_pre found all valid (results[0] == m), one
// workgroup per (solve, 1 KiB tile): the tile of every row is staged in LDS
// once, then wave w accumulates output rows w, w + 8, ... in registers, each
// source row's bytes split once into the multiply's bit groups and multiplied
// by every output row's coefficient T[r][k] (its v_perm tables fetched by
// scalar loads: the coefficient is uniform across the wave).  No pivot chain
// and no barrier after the staging, one LDS read per source row and wave,
// and no LDS writes: the sweeps read and wrote a row tile per row update and
// waited on a barrier per pivot step.  The workgroup owns its tile of every
// row of the solve, so it stores the results in place after reading them.
//
// Lane l holds the dwords at bytes 256 q + 4 l of the tile (q < 4): a tile
// that ends early (a 1402-byte row's second KiB has 378 bytes) skips the
// whole quarters past the solve's largest row, a quarter of the multiplies
// each instead of the idle lanes of 16-byte-per-lane tiles.
#ifndef SGPU_TR_WAVES
#define SGPU_TR_WAVES 8
#endif
#ifndef SGPU_TR_LDS_TABLES
#define SGPU_TR_LDS_TABLES 0
#endif
#ifndef SGPU_TR_SPLIT
#define SGPU_TR_SPLIT 1
#endif
constexpr unsigned kTrWaves = SGPU_TR_WAVES;
constexpr unsigned kTrSplit = SGPU_TR_SPLIT;            // workgroups per (solve, tile)
constexpr unsigned kTrStep = kTrWaves * kTrSplit;       // output row stride of a wave
constexpr unsigned kTrThreads = 64 * kTrWaves;
constexpr uint32_t kTrTableBytes = SGPU_TR_LDS_TABLES ? 256u * 20u : 0u;

// A workgroup takes half of a (solve, 1 KiB tile): m x 512 bytes of LDS, so
// the launch's largest solve (m <= 120) still leaves room for two or more
// workgroups per CU (a whole tile per workgroup, m KiB, ran one per CU:
// 512 workgroups in two rounds at 2 waves per SIMD)
constexpr unsigned kTrHalves = 2;
__host__ __device__ constexpr uint32_t solve_tr_lds_bytes(uint32_t m) { return kTrTableBytes + m * (1024u / kTrHalves); }

// a row's bytes in this workgroup's half tile: two dwords per lane
using TrRow = uint2;
__device__ __forceinline__ TrRow tr_row(const uint32_t (&v)[4]) { return make_uint2(v[0], v[1]); }
__device__ __forceinline__ void tr_unrow(TrRow r, uint32_t (&v)[4])
{
    v[0] = r.x;
    v[1] = r.y;
    v[2] = v[3] = 0;
}

template <unsigned NQ, unsigned RW>
__device__ __forceinline__ void solve_tr_tile(const SolveDesc& sd, const SolveRow* __restrict__ R,
                                              uint32_t* res, uint32_t tileBase,
                                              uint4* __restrict__ X)
{
    static_assert(NQ <= 4 / kTrHalves, "a workgroup's quarters of the tile");
    const uint32_t m = sd.m, tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
#if SGPU_TR_LDS_TABLES
    const uint4* permL = X;
    const uint32_t* permC = reinterpret_cast<const uint32_t*>(X + 256);
    if (tid < 256) {
        const uint32_t* t = c_perm[tid];
        X[tid] = make_uint4(t[0], t[1], t[2], t[3]);
        reinterpret_cast<uint32_t*>(X + 256)[tid] = t[4];
    }
    X += 256 + 64;
#endif
    TrRow* XR = reinterpret_cast<TrRow*>(X);
    // the tile of every row, bytes past a row's initial length as zero
    for (uint32_t j = wave; j < m; j += kTrWaves) {
        const uint64_t buf = R[j].buf;
        const uint32_t ib = R[j].initBytes;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (unsigned q = 0; q < NQ; ++q) {
            const uint32_t p = tileBase + 256u * q + 4u * lane;
            if (p < ib)
                v[q] = ld4(buf + p) & byte_mask((int)ib - (int)p);
        }
        XR[j * 64u + lane] = tr_row(v);
    }
    // this wave's rows of T (lane l < 32: bytes 4 l .. 4 l + 3 of each)
    // output rows r0 + kTrStep t of this wave (kTrSplit workgroups share a
    // tile, each its own rows)
    const uint32_t r0 = wave + kTrWaves * (kTrSplit > 1 ? (blockIdx.x / kTrHalves) % kTrSplit : 0u);
    const uint32_t rw = r0 < m ? (m - r0 + kTrStep - 1) / kTrStep : 0;
    uint32_t trow[RW];
#pragma unroll
    for (unsigned t = 0; t < RW; ++t)
        trow[t] = (t < rw && lane < kTStride / 4)
                      ? ld4(sd.tinv + (uint64_t)(r0 + kTrStep * t) * kTStride + 4u * lane)
                      : 0u;
    __syncthreads();

    uint32_t acc[RW][NQ];
#pragma unroll
    for (unsigned t = 0; t < RW; ++t)
#pragma unroll
        for (unsigned q = 0; q < NQ; ++q)
            acc[t][q] = 0;
    for (uint32_t k0 = 0; k0 < m; k0 += 4) {
        uint32_t tw[RW];
#pragma unroll
        for (unsigned t = 0; t < RW; ++t)
            tw[t] = rl(trow[t], k0 >> 2);   // T[r_t][k0 .. k0 + 3]
        const uint32_t kn = m - k0 < 4 ? m - k0 : 4;
        for (uint32_t kk = 0; kk < kn; ++kk) {
            uint32_t sv[4];
            tr_unrow(XR[(k0 + kk) * 64u + lane], sv);
            uint32_t sa[NQ], sb[NQ], sc[NQ];
#pragma unroll
            for (unsigned q = 0; q < NQ; ++q) {
                sa[q] = sv[q] & 0x07070707u;
                sb[q] = (sv[q] >> 3) & 0x07070707u;
                sc[q] = (sv[q] >> 6) & 0x03030303u;
            }
            // the tables of up to eight rows fetched together, then their
            // products, with no branch (RW = ceil(m / 8) or a little more: a
            // wave's rows past m have T zero, the table of 0, and are not
            // stored)
#pragma unroll
            for (unsigned t0 = 0; t0 < RW; t0 += 8) {
                constexpr unsigned kG = 8;
                GfTab tb[kG];
#pragma unroll
                for (unsigned u = 0; u < kG && t0 + u < RW; ++u)
#if SGPU_TR_LDS_TABLES
                    tb[u] = gf_tab_l(permL, permC, uni((tw[t0 + u] >> (8u * kk)) & 255u));
#else
                    tb[u] = gf_tab(uni((tw[t0 + u] >> (8u * kk)) & 255u));
#endif
#pragma unroll
                for (unsigned u = 0; u < kG && t0 + u < RW; ++u) {
#pragma unroll
                    for (unsigned q = 0; q < NQ; ++q) {
                        // (v_bitop3_b32 0x96 = three-way XOR: two XORs per
                        // product instead of three)
                        const uint32_t pa = __builtin_amdgcn_perm(tb[u].a1, tb[u].a0, sa[q]);
                        const uint32_t pb = __builtin_amdgcn_perm(tb[u].b1, tb[u].b0, sb[q]);
                        const uint32_t pc = __builtin_amdgcn_perm(0u, tb[u].c, sc[q]);
                        acc[t0 + u][q] = __builtin_amdgcn_bitop3_b32(acc[t0 + u][q], pa, pb, 0x96) ^ pc;
                    }
                }
            }
        }
    }
    // Into the scratch, masked past the recovered length, every 16-byte
    // chunk that starts below the row's final bytes (the chunks the exact
    // back-substitution stores).  A non-zero byte past a row's recovered
    // length flags the solve (res[m + 1]): the sweeps clip there, so the
    // tile pass redoes it the reference's way.
    const uint32_t xs = solve_x_stride(sd.maxBytes);
    uint32_t tail = 0;
#pragma unroll
    for (unsigned t = 0; t < RW; ++t) {
        if (t < rw) {
            const uint32_t i = r0 + kTrStep * t;
            const uint32_t w = res[1 + i];
            const uint32_t bb = (w >> 29) + (w & kSolveLengthMask), fb = R[i].finalBytes;
            const uint64_t out = sd.xout + (uint64_t)i * xs;
#pragma unroll
            for (unsigned q = 0; q < NQ; ++q) {
                const uint32_t p = tileBase + 256u * q + 4u * lane;
                const uint32_t keep = byte_mask((int)bb - (int)p);
                tail |= acc[t][q] & ~keep;
                if ((p & ~15u) < fb)
                    st4(out + p, acc[t][q] & keep);
            }
        }
    }
    if (__any(tail != 0) && lane == 0)
        atomicOr(res + 1 + m, 1u);
}

template <unsigned NQ>
__device__ __forceinline__ void solve_tr_rows(const SolveDesc& sd, const SolveRow* R, uint32_t* res,
                                              uint32_t tileBase, uint4* X)
{
    // output rows per wave: ceil(m / 8) <= 15 (m <= kProductMaxRows), rounded
    // up to one of these
    static_assert(kProductMaxRows <= 15 * kTrStep && kTrThreads <= 1024, "k_solve_tr keeps at most 15 rows per wave");
    const uint32_t rw = (sd.m + kTrStep - 1) / kTrStep;
    switch (rw) {
    case 1:
    case 2: solve_tr_tile<NQ, 2>(sd, R, res, tileBase, X); break;
    case 3:
    case 4: solve_tr_tile<NQ, 4>(sd, R, res, tileBase, X); break;
    case 5: solve_tr_tile<NQ, 5>(sd, R, res, tileBase, X); break;
    case 6: solve_tr_tile<NQ, 6>(sd, R, res, tileBase, X); break;
    case 7: solve_tr_tile<NQ, 7>(sd, R, res, tileBase, X); break;
    case 8: solve_tr_tile<NQ, 8>(sd, R, res, tileBase, X); break;
    case 9: solve_tr_tile<NQ, 9>(sd, R, res, tileBase, X); break;
    case 10: solve_tr_tile<NQ, 10>(sd, R, res, tileBase, X); break;
    case 11:
    case 12: solve_tr_tile<NQ, 12>(sd, R, res, tileBase, X); break;
    default: solve_tr_tile<NQ, 15>(sd, R, res, tileBase, X); break;
    }
}

__global__ __launch_bounds__(kTrThreads) void k_solve_tr(const SolveDesc* __restrict__ solves,
                                                         const SolveRow* __restrict__ rows,
                                                         uint32_t* results,
                                                         const SolveItem* __restrict__ items)
{
    extern __shared__ uint4 X[];
    const SolveItem it = items[blockIdx.x / (kTrSplit * kTrHalves)];
    const SolveDesc sd = solves[it.solve];
    const uint32_t tileBase = it.tileBase + (blockIdx.x % kTrHalves) * (1024u / kTrHalves);
    if (sd.m == 0 || sd.m > kProductMaxRows || sd.tinv == 0 || solve_gated_off(sd, results) ||
        results[sd.result] != sd.m || tileBase >= sd.maxBytes)
        return;   // (uniform: k_solve_main solves it, or the solve is gated off)
    const uint32_t left = sd.maxBytes - tileBase;
    const uint32_t nq = left >= 256u ? 2u : 1u;   // (quarters of this half)
    const SolveRow* R = rows + sd.rowBegin;
    uint32_t* res = results + sd.result;
    if (nq == 2)
        solve_tr_rows<2>(sd, R, res, tileBase, X);
    else
        solve_tr_rows<1>(sd, R, res, tileBase, X);
}

// ---------------------------------------------------------------------------
// The recovery matrix of a decode on the device (k_ge, ops.h GeDesc)
//
// One workgroup of eight waves per decode (a launch holds one job per CU: the
// job's own work must fill the CU's four SIMDs; a launch lasts as long as
// its largest matrix, so rows up to 128 take one pass), the matrix resident in LDS
// (ge_stride_words dwords a row: odd, so rows start in different banks) with
// the job's input staged beside it.  Generation (the host's generate_matrix;
// reference SiameseDecoder.cpp:2157-2383) writes four columns per thread: the
// dense part from the row's opcodes (Siamese), 1/(X ^ Y) (Cauchy) or 1
// (parity); then the LDPC picks, one row per wave and 64 PCG draws per pass
// (jump-ahead c_pcgA/c_pcgG), land by LDS XOR atomics.  The elimination is
// the reference's (:2423-2531): no pivoting while each pivot byte is
// non-zero, then row pivoting from the first zero one.  A pivot step is one
// pass and one barrier: four threads per row each take the row's multiplier
// y = row[p] / pivot and XOR y times a quarter of the pivot row's bytes
// (p, end) into it, their LDS reads all in flight.
// The GF(256) tables (multiply, inverse) are LDS copies: an inverse read from
// global memory on every pivot cost a memory round trip per pivot.
constexpr unsigned kGeThreads = 512;   // four threads for each of up to 128 rows a pass
constexpr unsigned kGePickLds = 4096;   // pick tables up to this many bytes are staged in LDS

__device__ __forceinline__ uint32_t ge_opcode(uint32_t lane, uint32_t row)
{
    // SiameseCommon.h:150-174 (wang_hash32 of lane + (row + 3) * 8, 0 -> 16)
    uint32_t k = lane + (row + 3u) * kLanes;
    k += ~(k << 15);
    k ^= k >> 10;
    k += k << 3;
    k ^= k >> 6;
    k += ~(k << 11);
    k ^= k >> 16;
    const uint32_t op = k & 63u;
    return op ? op : 16u;
}

__device__ __forceinline__ uint32_t ge_comb(uint32_t k, uint32_t cx, uint32_t cx2)
{
    return (k & 1u) ^ ((k & 2u) ? cx : 0u) ^ ((k & 4u) ? cx2 : 0u);
}

__host__ __device__ constexpr uint32_t ge_lds_bytes(uint32_t rows, uint32_t cols)
{
    return rows * ge_stride_words(cols) * 4u;
}


__global__ __launch_bounds__(kGeThreads) void k_ge(const GeDesc* __restrict__ descs, const uint8_t* __restrict__ in,
                                                  uint32_t* __restrict__ results, SolveRow* __restrict__ srows,
                                                  uint8_t* __restrict__ scoef, const SolveRow* __restrict__ srowsIn)
{
    extern __shared__ uint32_t M[];   // rows x S4 dwords
    __shared__ uint4 permL[256];
    __shared__ uint32_t permC[256];
    __shared__ uint32_t invL[64];     // GF(256) inverses, bytes
    __shared__ uint8_t piv[kGeMaxRows], used[kGeMaxRows];
    __shared__ uint8_t pivB[2][kGeMaxRows];   // the pivot order of pivoted steps (double-buffered)
    __shared__ uint16_t cnt[kGeMaxRows];
    __shared__ GeRow R[kGeMaxRows];
    __shared__ GeCol C[kGeMaxCols + 1];
    __shared__ uint8_t pickL[kGePickLds];
    __shared__ uint32_t foundL[3], nzL;
    __shared__ unsigned long long bytesL;
    __shared__ uint32_t srL[kGeMaxCols][6];   // a chained job's solve rows as they came (SolveRow)
    const uint8_t* invB = reinterpret_cast<const uint8_t*>(invL);
    uint8_t* Mb = reinterpret_cast<uint8_t*>(M);
#ifdef SGPU_GE_CLOCKS
    const unsigned long long gclk0 = wall_clock64();
#endif
    const GeDesc d = descs[blockIdx.x];
    const uint32_t rows = d.rows, cols = d.cols;
    const uint32_t S4 = ge_stride_words(cols), SB = 4u * S4;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const GeRow* Rg = reinterpret_cast<const GeRow*>(in + d.in);
    const GeCol* Cg = reinterpret_cast<const GeCol*>(Rg + rows);
    const uint8_t* pickG = reinterpret_cast<const uint8_t*>(Cg + cols);
    const bool pickStaged = d.pickLen <= kGePickLds;
    const uint8_t* pick = pickStaged ? pickL : pickG;

    // 0. staging: every load of the job's input and tables in flight at once
    if (tid < 256) {
        const uint32_t* t = c_perm[tid];
        permL[tid] = make_uint4(t[0], t[1], t[2], t[3]);
        permC[tid] = t[4];
    }
    if (tid < 64)
        invL[tid] = reinterpret_cast<const uint32_t*>(c_inv)[tid];
    if (tid < rows) {
        const GeRow g = Rg[tid];
        R[tid] = g;
        piv[tid] = (uint8_t)tid;
        used[tid] = 0;
        cnt[tid] = g.colCount;
    }
    if (tid < cols)
        C[tid] = Cg[tid];
    // (a chained job's solve rows, from wherever the upload's head is read:
    // they are rewritten in pivot order at the end)
    static_assert(sizeof(SolveRow) == 24, "SolveRow layout");
    if ((d.flags & kGeChained) && tid < cols) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(srowsIn + d.solveRow) + 6u * tid;
#pragma unroll
        for (unsigned k = 0; k < 6; ++k)
            srL[tid][k] = s[k];
    }
    if (pickStaged)
        for (uint32_t x = 4u * tid; x < d.pickLen; x += 4u * kGeThreads) {
            // (the pick table starts 4-byte aligned: GeRow 16 B, GeCol 4 B)
            const uint32_t v = *reinterpret_cast<const uint32_t*>(pickG + x);
            *reinterpret_cast<uint32_t*>(pickL + x) = v;
        }
    if (tid == 0) {
        bytesL = 0;
        nzL = 0;
        foundL[0] = foundL[1] = foundL[2] = 0xffffffffu;
    }
    // (the PCG jump-ahead constants of the picks, in registers before any
    // LDS atomic: loads past those are not hoisted out of the row loop)
    const uint64_t pcgJa = c_pcgA[lane], pcgJg = c_pcgG[lane];
    const uint64_t pcgA64 = c_pcgA[64], pcgG64 = c_pcgG[64];
    __syncthreads();
#ifdef SGPU_GE_CLOCKS
    const unsigned long long gclkS = wall_clock64();
#endif

    // 1. dense parts, a dword (four columns) per thread
    const uint32_t wpr = (cols + 3u) / 4u;
    for (uint32_t x = tid; x < rows * S4; x += kGeThreads) {
        const uint32_t r = x / S4, w = x - r * S4;
        uint32_t lo = 0;
        if (w < wpr) {
            const GeRow g = R[r];
            uint32_t hi = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t j = 4u * w + q;
                if (j < cols && j < g.jEnd) {
                    const GeCol c = C[j];
                    uint32_t v = 1u, h = 0u;
                    if (g.kind == GE_CAUCHY) {
                        v = invB[(uint8_t)(g.rbase ^ c.ccol)];
                    } else if (g.kind == GE_SIAMESE) {
                        const uint32_t op = ge_opcode(c.lane, g.row);
                        v = ge_comb(op & 7u, c.cx, c.cx2);
                        h = ge_comb(op >> 3, c.cx, c.cx2);
                    }
                    lo |= v << (8u * q);
                    hi |= h << (8u * q);
                }
            }
            if (hi)   // v ^ RX * h
                lo ^= gf_mul_tab(hi, gf_tab_l(permL, permC, 1u + (g.row + 1u) % kRowValuePeriod));
        }
        M[x] = lo;
    }
    __syncthreads();

    // 2. LDPC picks: one Siamese row per wave, draws c0 + lane per pass
    for (uint32_t r = wave; r < rows; r += kGeThreads / 64u) {
        const GeRow g = R[r];
        if (g.kind != GE_SIAMESE || g.ldpcN == 0)
            continue;   // (uniform in the wave)
        const uint32_t N = g.ldpcN, P = 2u * ((N + kPairRate - 1u) / kPairRate);
        const uint64_t inc = ((uint64_t)g.row << 1) | 1u;
        uint64_t sc = (inc + N) * kPcgMul + inc;   // state after Seed(row, N)
        const uint32_t rx = 1u + (g.row + 1u) % kRowValuePeriod;
        for (uint32_t c0 = 0; c0 < P; c0 += 64u) {
            const uint32_t k = c0 + lane;
            const uint64_t st = pcgJa * sc + inc * pcgJg;
            sc = pcgA64 * sc + inc * pcgG64;
            if (k < P) {
                const uint32_t col = pick[g.pickOff + pcg_output(st) % N];
                if (col < cols)
                    atomicXor(&M[r * S4 + col / 4u], ((k & 1u) ? rx : 1u) << (8u * (col & 3u)));
            }
        }
    }
    __syncthreads();
#ifdef SGPU_GE_CLOCKS
    const unsigned long long gclk1 = wall_clock64();
#endif

    // 3. elimination.  One pivot step: every row below `pivot` (through the
    // pivot order once pivoting) takes y = row[pivot] / val at [pivot], then
    // y * the source row's bytes (pivot, end) (SiameseDecoder.h:504-541).
    // Pivoted steps keep the pivot order in two buffers (step s reads
    // pivB[s & 1] and writes the order with its swap into the other) and find
    // the next pivot row while they update the rows: the first position at or
    // after pivot + 1 whose row holds a non-zero byte at column pivot + 1 goes
    // into foundL[(s + 1) % 3] (atomicMin); a step resets slot (s + 2) % 3,
    // read by step s - 1 before step s began.  One barrier a step, pivoted or
    // not.
    unsigned long long myBytes = 0;
    // (pivoted: position swapJ's row is swapRow, every other's order[k])
    auto eliminate = [&](uint32_t src, uint32_t pivot, uint32_t end, uint32_t val, const uint8_t* order,
                         uint32_t swapJ, uint32_t swapRow, uint32_t* detect) {
        // four threads per row (one wave holds whole rows): each takes the
        // row's multiplier y = row[pivot] / val itself (the quarter-0 thread
        // keeps it at [pivot]: the wave's reads of that byte come before its
        // store), then XORs y times its quarter of the pivot row's dwords
        // (pivot, end)
        const uint32_t w0 = (pivot + 1u) / 4u, w1 = (end + 3u) / 4u;
        const uint32_t per = end > pivot + 1u ? (w1 - w0 + 3u) / 4u : 0u;   // dwords a thread
        const uint32_t quarter = tid & 3u;
        const GfTab iv = gf_tab_l(permL, permC, invB[val]);
        // (the source row through a VGPR address: a uniform address is read
        // into scalars, one LDS round trip per dword)
        const uint32_t* S = M + opaque(src * S4);
        for (uint32_t k = pivot + 1u + (tid >> 2); k < rows; k += kGeThreads / 4u) {
            const uint32_t rk = order ? (k == swapJ ? swapRow : order[k]) : k;
            const uint32_t v = Mb[rk * SB + pivot];
            if (v) {
                const uint32_t y = gf_mul_tab(v, iv) & 0xffu;
                if (quarter == 0) {
                    Mb[rk * SB + pivot] = (uint8_t)y;
                    if (end > pivot + 1u)
                        myBytes += end - pivot - 1u;
                    if (order && cnt[rk] < end)
                        cnt[rk] = (uint16_t)end;
                }
                const uint32_t a = w0 + quarter * per;
                const uint32_t e = min(a + per, w1);
                const GfTab ty = gf_tab_l(permL, permC, y);
                uint32_t* D = M + rk * S4;
                for (uint32_t w = a; w < e; w += 4u) {
                    uint32_t sv[4], dv[4];
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) {
                        const uint32_t ww = w + q < e ? w + q : w;   // (in bounds, unused past e)
                        sv[q] = S[ww];
                        dv[q] = D[ww];
                    }
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) {
                        const uint32_t ww = w + q;
                        if (ww < e) {
                            const uint32_t mask = byte_mask((int)end - (int)(4u * ww)) &
                                                  ~byte_mask((int)(pivot + 1u) - (int)(4u * ww));
                            D[ww] = dv[q] ^ (gf_mul_tab(sv[q], ty) & mask);
                        }
                    }
                }
            }
            // (the row as this step leaves it: its quarters' stores came
            // before this read in the wave's instruction stream)
            if (detect && quarter == 0 && Mb[rk * SB + pivot + 1u])
                atomicMin(detect, k);
        }
        __syncthreads();   // (the next step reads the rows this one wrote)
    };
    uint32_t p = 0;
    for (; p < cols; ++p) {
        const uint32_t val = Mb[p * SB + p];
        if (val == 0)
            break;
        if (tid == 0)
            used[p] = 1;
        eliminate(p, p, cnt[p], val, nullptr, 0u, 0u, nullptr);
    }
    uint32_t stop = cols;
    if (p < cols) {
        // row p has a zero at column p: the first row after it with a non-zero
        for (uint32_t j = p + 1u + tid; j < rows; j += kGeThreads)
            if (Mb[j * SB + p])
                atomicMin(&foundL[p % 3u], j);
        for (uint32_t k = tid; k < rows; k += kGeThreads)
            pivB[p & 1u][k] = piv[k];
        __syncthreads();
        for (uint32_t pivot = p; pivot < cols; ++pivot) {
            const uint32_t j = foundL[pivot % 3u];
            const uint8_t* cur = pivB[pivot & 1u];
            uint8_t* nxt = pivB[(pivot & 1u) ^ 1u];
            if (j == 0xffffffffu) {
                stop = pivot;
                for (uint32_t k = tid; k < rows; k += kGeThreads)
                    piv[k] = cur[k];
                break;
            }
            const uint32_t rj = cur[j], rp = cur[pivot];
            // this step's order: the swap of positions pivot and j
            for (uint32_t k = tid; k < rows; k += kGeThreads)
                nxt[k] = k == j ? (uint8_t)rp : (k == pivot ? (uint8_t)rj : cur[k]);
            if (tid == 0) {
                used[rj] = 1;
                foundL[(pivot + 2u) % 3u] = 0xffffffffu;
            }
            if (pivot >= cols - 1u) {
                for (uint32_t k = tid; k < rows; k += kGeThreads)
                    piv[k] = k == j ? (uint8_t)rp : (k == pivot ? (uint8_t)rj : cur[k]);
                break;
            }
            // (the step reads the order as cur with the swap applied: nxt is
            // written during the step, for the next one)
            eliminate(rj, pivot, cnt[rj], Mb[rj * SB + pivot], cur, j, rp, &foundL[(pivot + 1u) % 3u]);
        }
    }
    __syncthreads();   // (the pivot order and the matrix as the elimination left them)
#ifdef SGPU_GE_CLOCKS
    const unsigned long long gclk2 = wall_clock64();
#endif

    // 4. outcome: the header words, the pivots, and for a chained job the
    // solve's coefficients and rows in pivot order; else the used rows, the
    // column counts and the matrix for the host to install
    const bool ok = stop == cols;
    const bool chained = (d.flags & kGeChained) != 0;
    // MultiplyLowerTriangle's multipliers: the eliminated matrix's non-zero
    // bytes below the diagonal, in pivot order (SiameseDecoder.cpp:1065-1104)
    uint32_t nz = 0;
    if (ok && tid < cols) {
        const uint8_t* row = Mb + piv[tid] * SB;
        for (uint32_t i = 0; i < tid; ++i)
            nz += row[i] != 0;
    }
#pragma unroll
    for (unsigned o = 32; o >= 1; o >>= 1) {
        myBytes += __shfl_xor(myBytes, o, 64);
        nz += __shfl_xor(nz, o, 64);
    }
    if (lane == 0) {
        if (myBytes)
            atomicAdd(&bytesL, myBytes);
        if (nz)
            atomicAdd(&nzL, nz);
    }
    __syncthreads();
    uint32_t* out = results + d.result;
    if (tid < kGeOutHeader) {
        const unsigned long long tb = bytesL;
#ifdef SGPU_GE_CLOCKS
        const uint32_t hdr[kGeOutHeader] = {stop, (uint32_t)tb, (uint32_t)(tb >> 32), ok ? 1u : 0u, nzL,
                                            (uint32_t)(gclkS - gclk0), (uint32_t)(gclk1 - gclkS),
                                            (uint32_t)(gclk2 - gclk1)};
#else
        const uint32_t hdr[kGeOutHeader] = {stop, (uint32_t)tb, (uint32_t)(tb >> 32), ok ? 1u : 0u, nzL, 0, 0, 0};
#endif
        uint32_t v = 0;
#pragma unroll
        for (unsigned k = 0; k < kGeOutHeader; ++k)
            v = tid == k ? hdr[k] : v;
        out[tid] = v;
    }
    for (uint32_t w = tid; w < (rows + 3u) / 4u; w += kGeThreads) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (4u * w + q < rows) {
                a |= (uint32_t)piv[4u * w + q] << (8u * q);
                b |= (uint32_t)used[4u * w + q] << (8u * q);
            }
        out[ge_out_pivots(rows) + w] = a;
        if (!chained)
            out[ge_out_used(rows) + w] = b;
    }
    if (chained) {
        if (!ok)
            return;   // (the gated items of the submission do not run)
        // coefficients: coef[j * cols + i] = the pivot-order row j's column i
        uint8_t* co = scoef + d.solveCoef;
        for (uint32_t x = tid; x < cols * cols; x += kGeThreads) {
            const uint32_t j = x / cols, i = x - j * cols;
            co[x] = Mb[piv[j] * SB + i];
        }
        // the solve's rows in pivot order, each keeping its head slot
        // (SolveRow: 6 dwords, the last the head slot), from their staged copy
        uint32_t* sr = reinterpret_cast<uint32_t*>(srows + d.solveRow);
        if (tid < cols) {
            const uint32_t src = piv[tid];
#pragma unroll
            for (unsigned k = 0; k < 5; ++k)
                sr[6u * tid + k] = srL[src][k];
            sr[6u * tid + 5] = 1u + solve_head_slot(srL[src][5], src);
        }
        return;
    }
    for (uint32_t w = tid; w < (rows + 1u) / 2u; w += kGeThreads)
        out[ge_out_counts(rows) + w] = (uint32_t)cnt[2u * w] | (2u * w + 1u < rows ? (uint32_t)cnt[2u * w + 1u] << 16 : 0u);
    const uint32_t total = rows * cols;
    for (uint32_t w = tid; w < (total + 3u) / 4u; w += kGeThreads) {
        uint32_t a = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t b = 4u * w + q;
            if (b < total) {
                const uint32_t r = b / cols;
                a |= (uint32_t)Mb[r * SB + (b - r * cols)] << (8u * q);
            }
        }
        out[ge_out_matrix(rows) + w] = a;
    }
}

// ---------------------------------------------------------------------------
// Delivery (k_deliver, ops.h DeliverItem)
//
// k_ingest run backwards: one wave per (item, 8 KiB chunk of its row), lane L
// of each 1 KiB tile writes row bytes [16L, 16L+16) with one 16-byte store.
// The wave reads the symbol's first aligned word, parses the length prefix
// (header h = 1..4 bytes, length L) and checks it against the symbol's
// readable bytes and the row; everything derived from it is wave-uniform.
// The payload starts at src + h, so a lane's 16 output bytes straddle the
// aligned source words at src + p and src + p + 16: both are loaded
// (coalesced) and recombined with v_alignbyte_b32, the shift chosen by a
// uniform branch on h.  A word is loaded only if the row needs a payload byte
// from it (p < L, and p + 16 < h + L for the second), which keeps every read
// inside the aligned words that hold a byte of [src, src + cap), since
// h + L <= cap.  Bytes at and past L are masked to zero and the zero fill
// runs to the row's end; rows and positions are 64-bit (rows of up to 4 GiB).
// Two tiles' loads are in flight before their stores.  No LDS, no atomics.

__global__ __launch_bounds__(64 * kDeliverWaves) void k_deliver(const DeliverItem* __restrict__ items,
                                                                uint32_t count)
{
    const uint32_t ii = __builtin_amdgcn_readfirstlane(blockIdx.x * kDeliverWaves + (threadIdx.x >> 6));
    if (ii >= count)
        return;
    const uint32_t lane = threadIdx.x & 63;
    const DeliverItem it = items[ii];
    const uint64_t stride = (uint64_t)it.stride16 << 4;
    uint32_t h = 0, L = 0;
    if (it.src != 0 && it.cap != 0) {   // (uniform)
        const uint32_t avail = it.cap < 4 ? it.cap : 4;
        const uint32_t w = __builtin_amdgcn_readfirstlane(ld16(it.src).x) & byte_mask((int)avail);
        uint32_t len = 0;
        const int hh = parse_prefix(w, avail, &len);
        if (hh >= 1 && len >= 1 && (uint32_t)hh + len <= it.cap && len <= stride) {
            h = (uint32_t)hh;
            L = len;
        }
    }
    if (blockIdx.y == 0 && lane == 0)
        *reinterpret_cast<GMEM uint32_t*>(it.lenOut) = L;
    if (it.src == 0)   // an absent packet: its row stays as it is
        return;
    const uint32_t end = h + L;   // symbol bytes in use (0: a zeroed row)
    const uint64_t step = (uint64_t)gridDim.y * kIngestChunkBytes;
    for (uint64_t c0 = (uint64_t)blockIdx.y * kIngestChunkBytes; c0 < stride; c0 += step) {
        const uint64_t c1 = c0 + kIngestChunkBytes < stride ? c0 + kIngestChunkBytes : stride;
        for (uint64_t t = c0; t < c1; t += 2 * kTileBytes) {
            uint4 out[2];
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                const uint4 lo = p < L ? ld16(it.src + p) : make_uint4(0, 0, 0, 0);
                const uint4 hi = p + 16 < end ? ld16(it.src + p + 16) : make_uint4(0, 0, 0, 0);
                const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                switch (h) {   // wave-uniform
                case 1:
                    out[u] = make_uint4(pick(w, 0, 1, 0), pick(w, 0, 1, 1), pick(w, 0, 1, 2), pick(w, 0, 1, 3));
                    break;
                case 2:
                    out[u] = make_uint4(pick(w, 0, 2, 0), pick(w, 0, 2, 1), pick(w, 0, 2, 2), pick(w, 0, 2, 3));
                    break;
                case 3:
                    out[u] = make_uint4(pick(w, 0, 3, 0), pick(w, 0, 3, 1), pick(w, 0, 3, 2), pick(w, 0, 3, 3));
                    break;
                default:   // h = 4 (or a zeroed row: nothing was loaded)
                    out[u] = make_uint4(w[1], w[2], w[3], w[4]);
                    break;
                }
            }
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                if (p >= stride)
                    continue;
                uint4 v = out[u];
                if (p + 16 > L)
                    v = mask16(v, p < L ? (int)(L - (uint32_t)p) : 0);
                st16(it.dst + p, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Framing (k_frame, ops.h FrameItem)
//
// k_deliver's shape for the sender's packets: one wave per (item, 8 KiB chunk
// of its row), lane L of each 1 KiB tile writes row bytes [16L, 16L+16) with
// one 16-byte store.  Nothing is parsed on the device: the host knows every
// length, so the row's content is T = hdrLen + bytes, a literal header of up
// to 11 bytes and then the packet from src, which has any byte alignment.
// The source byte that lines up with row byte 0 is src - hdrLen; its low four
// bits give a word offset and a byte shift that are uniform per item, so a
// lane's 16 bytes come from the two aligned source words around them, loaded
// (coalesced) and recombined with v_alignbyte_b32 under a uniform branch, as
// in k_ingest.  An aligned word is loaded only if it holds a byte of
// [src, src + bytes) (the second word of the first lane always does when the
// first lies before src: hdrLen < 16).  The header bytes are merged into
// lane 0 of tile 0, bytes at and past T are masked to zero and the zero fill
// runs to the row's end; positions are 64-bit.  Two tiles' loads are in
// flight before their stores.  No LDS, no atomics.

__global__ __launch_bounds__(64 * kDeliverWaves) void k_frame(const FrameItem* __restrict__ items, uint32_t count)
{
    const uint32_t ii = __builtin_amdgcn_readfirstlane(blockIdx.x * kDeliverWaves + (threadIdx.x >> 6));
    if (ii >= count)
        return;
    const uint32_t lane = threadIdx.x & 63;
    const FrameItem it = items[ii];
    const uint64_t stride = (uint64_t)it.stride16 << 4;
    const uint32_t hl = it.hdrLen;
    const uint64_t total = it.src != 0 ? (uint64_t)hl + it.bytes : 0;   // (<= stride: the host checked)
    if (blockIdx.y == 0 && lane == 0 && it.lenOut != 0)   // (none: not the last frame of a packed row)
        *reinterpret_cast<GMEM uint32_t*>(it.lenOut) = it.lenBase + (uint32_t)total;
    if (it.src == 0)   // an absent packet: its row stays as it is
        return;
    // source address that lines up with row byte 0
    const uint64_t base = it.src - hl;
    const unsigned sh = (unsigned)(base & 15u);
    const unsigned q = sh >> 2, r = sh & 3;
    const uint64_t srcEnd = it.src + it.bytes;
    const bool any = it.bytes != 0;
    const uint32_t h0 = it.hdr[0] | (it.hdr[1] << 8) | (it.hdr[2] << 16) | ((uint32_t)it.hdr[3] << 24);
    const uint32_t h1 = it.hdr[4] | (it.hdr[5] << 8) | (it.hdr[6] << 16) | ((uint32_t)it.hdr[7] << 24);
    const uint32_t h2 = it.hdr[8] | (it.hdr[9] << 8) | (it.hdr[10] << 16);
    const uint64_t step = (uint64_t)gridDim.y * kIngestChunkBytes;
    for (uint64_t c0 = (uint64_t)blockIdx.y * kIngestChunkBytes; c0 < stride; c0 += step) {
        const uint64_t c1 = c0 + kIngestChunkBytes < stride ? c0 + kIngestChunkBytes : stride;
        for (uint64_t t = c0; t < c1; t += 2 * kTileBytes) {
            uint4 out[2];
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                out[u] = make_uint4(0, 0, 0, 0);
                if (p >= total)   // the zero fill: nothing to load
                    continue;
                const uint64_t a = (base + p) & ~(uint64_t)15;
                const uint4 lo = (any && a < srcEnd && a + 16 > it.src) ? ld16(a) : make_uint4(0, 0, 0, 0);
                const uint4 hi = (any && sh != 0 && a + 16 < srcEnd) ? ld16(a + 16) : make_uint4(0, 0, 0, 0);
                const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                switch (q) {   // wave-uniform
                case 0:
                    out[u] = make_uint4(pick(w, 0, r, 0), pick(w, 0, r, 1), pick(w, 0, r, 2), pick(w, 0, r, 3));
                    break;
                case 1:
                    out[u] = make_uint4(pick(w, 1, r, 0), pick(w, 1, r, 1), pick(w, 1, r, 2), pick(w, 1, r, 3));
                    break;
                case 2:
                    out[u] = make_uint4(pick(w, 2, r, 0), pick(w, 2, r, 1), pick(w, 2, r, 2), pick(w, 2, r, 3));
                    break;
                default:
                    out[u] = make_uint4(pick(w, 3, r, 0), pick(w, 3, r, 1), pick(w, 3, r, 2), pick(w, 3, r, 3));
                    break;
                }
            }
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                if (p >= stride)
                    continue;
                uint4 v = out[u];
                if (p == 0) {   // the frame header (at most 11 bytes) over source bytes
                    const uint32_t m0 = byte_mask((int)hl), m1 = byte_mask((int)hl - 4), m2 = byte_mask((int)hl - 8);
                    v.x = (v.x & ~m0) | (h0 & m0);
                    v.y = (v.y & ~m1) | (h1 & m1);
                    v.z = (v.z & ~m2) | (h2 & m2);
                }
                if (p + 16 > total)
                    v = mask16(v, p < total ? (int)(total - p) : 0);
                st16(it.dst + p, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Relay (k_relay, ops.h RelayItem)
//
// k_deliver's parse in front of k_frame's copy: one wave per (item, 8 KiB
// chunk of its row), lane L of each 1 KiB tile writes row bytes [16L, 16L+16)
// with one 16-byte store.  The wave reads the symbol's first aligned word and
// parses its length prefix (hs = 1..4 bytes, length n) as k_deliver does; the
// frame's own prefix is that of L = n + 7 (1 byte below 0x80, 2 below 0x4000,
// 3 below 0x200000, else 4: write_length_prefix's bit patterns), followed by
// type 0, three flow bytes and three PacketNum bytes, hf = 8..11 bytes held in
// three dwords.  All of it is wave-uniform.  The packet fits when n >= 1,
// hs + n <= cap, L fits a prefix and hf + n <= stride (frames.h relay_fits);
// otherwise the row is zero and its length 0.  Row byte p is symbol byte
// p - hf + hs, so the source address that lines up with row byte 0 is
// src + hs - hf: src is 16-byte aligned and hs - hf lies in [-10, -4], so the
// byte shift (6..12) is never zero and every lane's 16 bytes straddle two
// aligned source words, loaded (coalesced) only if they hold a byte of
// [src + hs, src + hs + n) and recombined with v_alignbyte_b32 under a uniform
// branch, as in k_frame.  The header is merged into lane 0 of tile 0, bytes at
// and past hf + n are masked to zero and the zero fill runs to the row's end;
// positions are 64-bit.  Two tiles' loads are in flight before their stores.
// No LDS, no atomics.

__global__ __launch_bounds__(64 * kDeliverWaves) void k_relay(const RelayItem* __restrict__ items, uint32_t count)
{
    const uint32_t ii = __builtin_amdgcn_readfirstlane(blockIdx.x * kDeliverWaves + (threadIdx.x >> 6));
    if (ii >= count)
        return;
    const uint32_t lane = threadIdx.x & 63;
    const RelayItem it = items[ii];
    const uint64_t stride = (uint64_t)it.stride16 << 4;
    uint32_t hs = 0, hf = 0, n = 0;
    uint32_t h0 = 0, h1 = 0, h2 = 0;   // the frame header, little-endian dwords
    if (it.src != 0 && it.cap != 0) {   // (uniform)
        const uint32_t avail = it.cap < 4 ? it.cap : 4;
        const uint32_t w = __builtin_amdgcn_readfirstlane(ld16(it.src).x) & byte_mask((int)avail);
        uint32_t len = 0;
        const int hh = parse_prefix(w, avail, &len);
        if (hh >= 1 && len >= 1 && (uint32_t)hh + len <= it.cap && len + 7u <= kFrameMaxLength) {
            const uint32_t Lf = len + 7u;   // type, flow, PacketNum, payload
            uint32_t pf, pre;               // the frame's prefix: bytes, and the bytes as a little-endian dword
            if (Lf < 0x80u) {
                pf = 1;
                pre = Lf;
            } else if (Lf < 0x4000u) {
                pf = 2;
                pre = (0x80u | (Lf >> 8)) | ((Lf & 0xffu) << 8);
            } else if (Lf < 0x200000u) {
                pf = 3;
                pre = (0xC0u | (Lf >> 16)) | (((Lf >> 8) & 0xffu) << 8) | ((Lf & 0xffu) << 16);
            } else {
                pf = 4;
                pre = (0xE0u | (Lf >> 24)) | (((Lf >> 16) & 0xffu) << 8) | (((Lf >> 8) & 0xffu) << 16) |
                      ((Lf & 0xffu) << 24);
            }
            if ((uint64_t)pf + Lf <= stride) {
                hs = (uint32_t)hh;
                n = len;
                hf = pf + 7u;
                // type 0, flow and PacketNum as 56 bits behind the prefix
                const uint64_t body = ((uint64_t)(it.flow & 0xffffffu) << 8) | ((uint64_t)(it.packetNum & 0xffffffu) << 32);
                const uint32_t s = 8u * pf;   // 8..32
                const uint64_t lo = (uint64_t)pre | (body << s);
                h0 = (uint32_t)lo;
                h1 = (uint32_t)(lo >> 32);
                h2 = (uint32_t)(body >> (64u - s));
            }
        }
    }
    const uint64_t total = (uint64_t)hf + n;   // row bytes in use (0: a zeroed row)
    if (blockIdx.y == 0 && lane == 0)
        *reinterpret_cast<GMEM uint32_t*>(it.lenOut) = (uint32_t)total;
    if (it.src == 0)   // an absent packet: its row stays as it is
        return;
    // source address that lines up with row byte 0, and the payload's span
    const uint64_t src = it.src + hs;
    const uint64_t base = src - hf;
    const unsigned sh = (unsigned)(base & 15u);   // 6..12 (0 for a zeroed row: nothing is loaded)
    const unsigned q = sh >> 2, r = sh & 3;
    const uint64_t srcEnd = src + n;
    const uint64_t step = (uint64_t)gridDim.y * kIngestChunkBytes;
    for (uint64_t c0 = (uint64_t)blockIdx.y * kIngestChunkBytes; c0 < stride; c0 += step) {
        const uint64_t c1 = c0 + kIngestChunkBytes < stride ? c0 + kIngestChunkBytes : stride;
        for (uint64_t t = c0; t < c1; t += 2 * kTileBytes) {
            uint4 out[2];
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                out[u] = make_uint4(0, 0, 0, 0);
                if (p >= total)   // the zero fill: nothing to load
                    continue;
                const uint64_t a = (base + p) & ~(uint64_t)15;
                const uint4 lo = (a < srcEnd && a + 16 > src) ? ld16(a) : make_uint4(0, 0, 0, 0);
                const uint4 hi = a + 16 < srcEnd ? ld16(a + 16) : make_uint4(0, 0, 0, 0);
                const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                switch (q) {   // wave-uniform; 1..3 for a row in use
                case 1:
                    out[u] = make_uint4(pick(w, 1, r, 0), pick(w, 1, r, 1), pick(w, 1, r, 2), pick(w, 1, r, 3));
                    break;
                case 2:
                    out[u] = make_uint4(pick(w, 2, r, 0), pick(w, 2, r, 1), pick(w, 2, r, 2), pick(w, 2, r, 3));
                    break;
                default:
                    out[u] = make_uint4(pick(w, 3, r, 0), pick(w, 3, r, 1), pick(w, 3, r, 2), pick(w, 3, r, 3));
                    break;
                }
            }
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                if (p >= stride)
                    continue;
                uint4 v = out[u];
                if (p == 0) {   // the frame header (8..11 bytes; none for a zeroed row) over source bytes
                    const uint32_t m0 = byte_mask((int)hf), m1 = byte_mask((int)hf - 4), m2 = byte_mask((int)hf - 8);
                    v.x = (v.x & ~m0) | (h0 & m0);
                    v.y = (v.y & ~m1) | (h1 & m1);
                    v.z = (v.z & ~m2) | (h2 & m2);
                }
                if (p + 16 > total)
                    v = mask16(v, p < total ? (int)(total - p) : 0);
                st16(it.dst + p, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Relay into packed rows (k_plan and k_pack; ops.h PackJob, PackItem, PlanRec)
//
// k_relay with several frames to a row.  Where a frame goes depends on the
// length of every frame before it, and the length of a packet recovered in
// this submission exists only here, so the layout is made on the device:
// k_plan runs the packer's cursor rule (frames.h pack_plan) over the lengths
// and leaves one 16-byte record per item, k_pack is k_relay's copy with the
// destination, the span to fill and the item's validity taken from its record.

// k_relay's test on one symbol (frames.h relay_fits): w = the symbol's first
// dword, cap its readable bytes, limit the bytes the frame may take.  Returns
// the frame's own prefix bytes (1..4: the frame is pf + 7 + *n bytes), or 0
// with *hs = *n = 0 for a packet that does not fit.
__device__ __forceinline__ uint32_t relay_sizes(uint32_t w, uint32_t cap, uint64_t limit, uint32_t* hs, uint32_t* n)
{
    *hs = 0;
    *n = 0;
    if (cap == 0)
        return 0;
    const uint32_t avail = cap < 4 ? cap : 4;
    uint32_t len = 0;
    const int hh = parse_prefix(w & byte_mask((int)avail), avail, &len);
    if (hh < 1 || len < 1 || (uint32_t)hh + len > cap || len + 7u > kFrameMaxLength)
        return 0;
    const uint32_t Lf = len + 7u;   // type, flow, PacketNum, payload
    const uint32_t pf = Lf < 0x80u ? 1u : Lf < 0x4000u ? 2u : Lf < 0x200000u ? 3u : 4u;
    if ((uint64_t)pf + Lf > limit)
        return 0;
    *hs = (uint32_t)hh;
    *n = len;
    return pf;
}

// k_plan: one wave per job.  64 items at a time, lane L reads item b + L's
// first symbol dword (a 4-byte load at the 16-byte aligned symbol) and computes
// its frame's bytes T, 0 for an absent packet or one that does not fit; such
// an item's record is zero and is stored by its own lane.  The wave then walks
// the frames among the 64 in order -- the set bits of the ballot of T != 0,
// each T fetched with v_readlane -- with the cursor (row, off) and the counters
// in scalar registers.  A frame's span is known when the next frame is placed,
// so each step stores the record of the frame before it, and that frame's
// row's length word when the row changed, from lane 0; the last frame's follow
// the loop.  Every row below the layout's row count holds a frame, so the
// length words of rows [min(rows, maxRows), maxRows) are the ones left to zero,
// 64 per store.  The walk is serial: one step per frame, a few tens of scalar
// instructions and at most two one-lane stores, at most 65535 steps a job;
// jobs run side by side.  No LDS, no atomics, no scratch.
__global__ __launch_bounds__(64 * kDeliverWaves) void k_plan(const PackJob* __restrict__ jobs, uint32_t jobCount,
                                                             const PackItem* __restrict__ items,
                                                             PlanRec* __restrict__ plan)
{
    const uint32_t ji = __builtin_amdgcn_readfirstlane(blockIdx.x * kDeliverWaves + (threadIdx.x >> 6));
    if (ji >= jobCount)
        return;
    const uint32_t lane = threadIdx.x & 63;
    const PackJob jb = jobs[ji];
    const uint64_t stride = (uint64_t)jb.stride16 << 4;
    const uint64_t planBase = (uint64_t)(uintptr_t)(plan + jb.first);
    uint32_t row = 0, frames = 0, written = 0, unfit = 0;
    uint64_t off = 0;
    bool open = false;   // a frame was placed whose record is not stored yet
    uint32_t prevK = 0, prevRow = 0;
    uint64_t prevOff = 0, prevEnd = 0;
    for (uint32_t b = 0; b < jb.count; b += 64) {
        const uint32_t k = b + lane;
        uint32_t T = 0;
        bool present = false;
        if (k < jb.count) {
            const PackItem it = items[jb.first + k];
            present = it.src != 0;
            if (present && it.cap != 0) {
                uint32_t hs, n;
                const uint32_t pf = relay_sizes(*reinterpret_cast<const GMEM uint32_t*>(it.src), it.cap, stride, &hs, &n);
                T = pf ? pf + 7u + n : 0u;
            }
            if (T == 0)
                st16(planBase + (uint64_t)k * sizeof(PlanRec), make_uint4(0, 0, 0, 0));
        }
        unfit += (uint32_t)__popcll(__ballot(present && T == 0));
        uint64_t m = __ballot(T != 0);
        while (m) {   // (wave-uniform)
            const uint32_t j = __builtin_amdgcn_readfirstlane((uint32_t)__builtin_ctzll(m));
            m &= m - 1;
            const uint32_t Tj = __builtin_amdgcn_readlane(T, j);
            if (off + Tj > stride) {
                ++row;
                off = 0;
            }
            if (open && lane == 0) {
                const uint64_t span = (prevRow == row ? off : stride) - prevOff;
                st16(planBase + (uint64_t)prevK * sizeof(PlanRec),
                     make_uint4(prevRow, (uint32_t)(prevOff >> 4), (uint32_t)(span >> 4),
                                prevRow < jb.maxRows ? kPlanWrite : 0u));
                if (prevRow != row && prevRow < jb.maxRows)
                    *reinterpret_cast<GMEM uint32_t*>(jb.lens + (uint64_t)prevRow * 4) = (uint32_t)prevEnd;
            }
            written += row < jb.maxRows ? 1u : 0u;
            ++frames;
            open = true;
            prevK = b + j;
            prevRow = row;
            prevOff = off;
            prevEnd = off + Tj;
            off = (prevEnd + 15) & ~(uint64_t)15;
        }
    }
    if (open && lane == 0) {
        st16(planBase + (uint64_t)prevK * sizeof(PlanRec),
             make_uint4(prevRow, (uint32_t)(prevOff >> 4), (uint32_t)((stride - prevOff) >> 4),
                        prevRow < jb.maxRows ? kPlanWrite : 0u));
        if (prevRow < jb.maxRows)
            *reinterpret_cast<GMEM uint32_t*>(jb.lens + (uint64_t)prevRow * 4) = (uint32_t)prevEnd;
    }
    const uint32_t rows = frames ? row + 1 : 0;
    for (uint64_t r = (uint64_t)(rows < jb.maxRows ? rows : jb.maxRows) + lane; r < jb.maxRows; r += 64)
        *reinterpret_cast<GMEM uint32_t*>(jb.lens + r * 4) = 0;
    if (lane == 0)
        st16(jb.info, make_uint4(rows, written, unfit, frames - written));
}

// k_pack: k_relay's grid and copy -- one wave per (item, 8 KiB chunk of its
// span), lane L of each 1 KiB tile writing span bytes [16L, 16L+16) with one
// 16-byte store, the header merged into lane 0 of tile 0 in registers, the
// payload byte-shifted with v_alignbyte_b32, zeros from the frame's end to the
// span's end -- with dst = rows + row * stride + 16 * off16 and the span in
// place of the row, both from the item's plan record; an item without
// kPlanWrite is left alone.  The source shift is that of k_relay: the symbol
// and dst are both 16-byte aligned (rows, stride and the offset are multiples
// of 16), so span byte 0 lines up with src + hs - hf, hs - hf in [-10, -4], the
// shift is 6..12 and the three cases of q are the ones that occur.  The plan
// admitted the frame under the row's stride and a span holds its frame, so
// the test against the span passes for every record k_plan flagged; were the
// symbol to differ from what k_plan read, the span would be zeroed as k_relay
// zeroes a row.  No LDS, no atomics, no scratch.
__global__ __launch_bounds__(64 * kDeliverWaves) void k_pack(const PackJob* __restrict__ jobs,
                                                             const PackItem* __restrict__ items,
                                                             const PlanRec* __restrict__ plan, uint32_t count)
{
    const uint32_t ii = __builtin_amdgcn_readfirstlane(blockIdx.x * kDeliverWaves + (threadIdx.x >> 6));
    if (ii >= count)
        return;
    const uint32_t lane = threadIdx.x & 63;
    const PlanRec pr = plan[ii];
    if (!(pr.flags & kPlanWrite))   // (uniform)
        return;
    const PackItem it = items[ii];
    const PackJob jb = jobs[it.job];
    const uint64_t span = (uint64_t)pr.span16 << 4;
    const uint64_t dst = jb.rows + (uint64_t)pr.row * ((uint64_t)jb.stride16 << 4) + ((uint64_t)pr.off16 << 4);
    uint32_t hs = 0, hf = 0, n = 0;
    uint32_t h0 = 0, h1 = 0, h2 = 0;   // the frame header, little-endian dwords
    {
        const uint32_t w = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const GMEM uint32_t*>(it.src));
        const uint32_t pf = relay_sizes(w, it.cap, span, &hs, &n);
        if (pf) {
            const uint32_t Lf = n + 7u;
            const uint32_t pre = pf == 1   ? Lf
                                 : pf == 2 ? (0x80u | (Lf >> 8)) | ((Lf & 0xffu) << 8)
                                 : pf == 3 ? (0xC0u | (Lf >> 16)) | (((Lf >> 8) & 0xffu) << 8) | ((Lf & 0xffu) << 16)
                                           : (0xE0u | (Lf >> 24)) | (((Lf >> 16) & 0xffu) << 8) |
                                                 (((Lf >> 8) & 0xffu) << 16) | ((Lf & 0xffu) << 24);
            hf = pf + 7u;
            // type 0, flow and PacketNum as 56 bits behind the prefix
            const uint64_t body = ((uint64_t)(it.flow & 0xffffffu) << 8) | ((uint64_t)(it.packetNum & 0xffffffu) << 32);
            const uint32_t s = 8u * pf;   // 8..32
            const uint64_t lo = (uint64_t)pre | (body << s);
            h0 = (uint32_t)lo;
            h1 = (uint32_t)(lo >> 32);
            h2 = (uint32_t)(body >> (64u - s));
        }
    }
    const uint64_t total = (uint64_t)hf + n;   // span bytes in use
    const uint64_t src = it.src + hs;
    const uint64_t base = src - hf;
    const unsigned sh = (unsigned)(base & 15u);   // 6..12 (0 for a zeroed span: nothing is loaded)
    const unsigned q = sh >> 2, r = sh & 3;
    const uint64_t srcEnd = src + n;
    const uint64_t step = (uint64_t)gridDim.y * kIngestChunkBytes;
    for (uint64_t c0 = (uint64_t)blockIdx.y * kIngestChunkBytes; c0 < span; c0 += step) {
        const uint64_t c1 = c0 + kIngestChunkBytes < span ? c0 + kIngestChunkBytes : span;
        for (uint64_t t = c0; t < c1; t += 2 * kTileBytes) {
            uint4 out[2];
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                out[u] = make_uint4(0, 0, 0, 0);
                if (p >= total)   // the zero fill: nothing to load
                    continue;
                const uint64_t a = (base + p) & ~(uint64_t)15;
                const uint4 lo = (a < srcEnd && a + 16 > src) ? ld16(a) : make_uint4(0, 0, 0, 0);
                const uint4 hi = a + 16 < srcEnd ? ld16(a + 16) : make_uint4(0, 0, 0, 0);
                const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                switch (q) {   // wave-uniform; 1..3 for a span in use
                case 1:
                    out[u] = make_uint4(pick(w, 1, r, 0), pick(w, 1, r, 1), pick(w, 1, r, 2), pick(w, 1, r, 3));
                    break;
                case 2:
                    out[u] = make_uint4(pick(w, 2, r, 0), pick(w, 2, r, 1), pick(w, 2, r, 2), pick(w, 2, r, 3));
                    break;
                default:
                    out[u] = make_uint4(pick(w, 3, r, 0), pick(w, 3, r, 1), pick(w, 3, r, 2), pick(w, 3, r, 3));
                    break;
                }
            }
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                if (p >= span)
                    continue;
                uint4 v = out[u];
                if (p == 0) {   // the frame header (8..11 bytes) over source bytes
                    const uint32_t m0 = byte_mask((int)hf), m1 = byte_mask((int)hf - 4), m2 = byte_mask((int)hf - 8);
                    v.x = (v.x & ~m0) | (h0 & m0);
                    v.y = (v.y & ~m1) | (h1 & m1);
                    v.z = (v.z & ~m2) | (h2 & m2);
                }
                if (p + 16 > total)
                    v = mask16(v, p < total ? (int)(total - p) : 0);
                st16(dst + p, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Delivery as a byte stream (k_offsets and k_concat; ops.h ConcatJob,
// ConcatItem, ConcatRec)
//
// k_deliver without rows: the payloads back to back at byte offsets.  An
// offset is the sum of every length before it, and the length of a packet
// recovered in this submission exists only here, so the sum is made on the
// device (frames.h concat_plan); the cursor has no row turn, so it is a plain
// prefix sum and needs no serial walk.

// k_offsets: one wave per job.  64 positions at a time, lane L takes position
// k = b + L: an item (k < count) reads its first symbol dword (a 4-byte load at
// the 16-byte aligned symbol) and computes n as k_deliver does, 0 for an
// invalid packet; a position that is no item has n = 0.  The wave takes the
// inclusive sum of n over its lanes (six __shfl_up steps, on 64-bit values:
// 64 lengths of up to 2^29 - 1 pass 2^32) on top of the running sum of the
// passes before, which is wave-uniform and 64-bit for the same reason.  A lane
// stops the stream when it is no item, when its n is 0 or when its sum passes
// the capacity; the first such lane, ctz of the ballot, is d, its exclusive sum
// is B (every lane before it fits, so B <= capacity < 2^32) and its kind is the
// stop reason.  Position count is no item, so every job stops.  Lanes before
// the stop store their offset word and a record flagged kConcatWrite, lanes at
// and behind it store B and a zero record, and the passes after the stop only
// store.  Lane 0 writes the info record with one 16-byte store.  No LDS, no
// atomics, no scratch.
__global__ __launch_bounds__(64 * kDeliverWaves) void k_offsets(const ConcatJob* __restrict__ jobs, uint32_t jobCount,
                                                                const ConcatItem* __restrict__ items,
                                                                ConcatRec* __restrict__ recs)
{
    const uint32_t ji = __builtin_amdgcn_readfirstlane(blockIdx.x * kDeliverWaves + (threadIdx.x >> 6));
    if (ji >= jobCount)
        return;
    const uint32_t lane = threadIdx.x & 63;
    const ConcatJob jb = jobs[ji];
    const uint64_t recBase = (uint64_t)(uintptr_t)(recs + jb.first);
    uint64_t carry = 0;   // the sum of the passes before (wave-uniform)
    bool stopped = false;
    uint32_t d = 0, B = 0, stop = 0;
    for (uint32_t b = 0; b <= jb.total; b += 64) {
        const uint32_t k = b + lane;
        const bool item = k < jb.count;
        uint32_t n = 0, hs = 0, off = 0;
        bool live = false;   // this lane's packet is delivered
        if (!stopped) {      // (wave-uniform)
            if (item) {
                const ConcatItem it = items[jb.first + k];
                if (it.cap != 0) {
                    const uint32_t avail = it.cap < 4 ? it.cap : 4;
                    const uint32_t w = *reinterpret_cast<const GMEM uint32_t*>(it.src) & byte_mask((int)avail);
                    uint32_t len = 0;
                    const int hh = parse_prefix(w, avail, &len);
                    if (hh >= 1 && len >= 1 && (uint32_t)hh + len <= it.cap) {
                        hs = (uint32_t)hh;
                        n = len;
                    }
                }
            }
            uint32_t lo = n, hi = 0;
#pragma unroll
            for (unsigned s = 1; s < 64; s <<= 1) {
                const uint32_t ulo = __shfl_up(lo, s), uhi = __shfl_up(hi, s);
                if (lane >= s) {
                    const uint64_t v = (((uint64_t)hi << 32) | lo) + (((uint64_t)uhi << 32) | ulo);
                    lo = (uint32_t)v;
                    hi = (uint32_t)(v >> 32);
                }
            }
            const uint64_t incl = carry + (((uint64_t)hi << 32) | lo);
            off = (uint32_t)(incl - n);   // (exact for every lane before the stop)
            const uint64_t m = __ballot(!item || n == 0 || incl > (uint64_t)jb.capacity);
            if (m) {
                const uint32_t j = __builtin_amdgcn_readfirstlane((uint32_t)__builtin_ctzll(m));
                stopped = true;
                d = b + j;
                B = __builtin_amdgcn_readlane(off, j);
                stop = d >= jb.count ? 0u : __builtin_amdgcn_readlane(n, j) == 0 ? 1u : 2u;
                live = lane < j;
            } else {
                live = true;
                carry = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(incl >> 32), 63) << 32) |
                        __builtin_amdgcn_readlane((uint32_t)incl, 63);
            }
        }
        if (k <= jb.total)
            *reinterpret_cast<GMEM uint32_t*>(jb.offsets + (uint64_t)k * 4) = live ? off : B;
        if (item)
            st16(recBase + (uint64_t)k * sizeof(ConcatRec),
                 live ? make_uint4(off, n, hs, kConcatWrite) : make_uint4(0, 0, 0, 0));
    }
    if (lane == 0)
        st16(jb.info, make_uint4(d, B, stop, jb.count));
}

// The bytes [b0, b1) of the aligned 16-byte word at `a`, from v, with stores no
// wider than the bytes owned: a dword where all four are, else a short where
// both are, else the byte.  The word's other bytes belong to a neighbouring
// packet, whose wave writes them in the same launch, or to the caller: they are
// neither read nor written.
__device__ __forceinline__ void st_bytes(uint64_t a, uint4 v, uint32_t b0, uint32_t b1)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (unsigned i = 0; i < 4; ++i) {
        const uint32_t at = 4 * i;
        if (b0 <= at && at + 4 <= b1) {
            *reinterpret_cast<GMEM uint32_t*>(a + at) = w[i];
            continue;
        }
#pragma unroll
        for (unsigned h = 0; h < 2; ++h) {
            const uint32_t a2 = at + 2 * h;
            const uint32_t y = w[i] >> (16 * h);
            if (b0 <= a2 && a2 + 2 <= b1) {
                *reinterpret_cast<GMEM uint16_t*>(a + a2) = (uint16_t)y;
            } else {
                if (b0 <= a2 && a2 < b1)
                    *reinterpret_cast<GMEM uint8_t*>(a + a2) = (uint8_t)y;
                if (b0 <= a2 + 1 && a2 + 1 < b1)
                    *reinterpret_cast<GMEM uint8_t*>(a + a2 + 1) = (uint8_t)(y >> 8);
            }
        }
    }
}

// k_concat: k_deliver's grid -- one wave per (item, 8 KiB chunk) -- over the
// aligned 16-byte words of the destination that hold a byte of the payload.
// D = dst + off has any alignment; positions p count from A0 = D rounded down
// to 16, the payload is [dlo, dlo + n) there and lane L of each 1 KiB tile owns
// the word at p = 16 L.  A word wholly inside the payload (the body) is one
// 16-byte store.  The first and the last word may be partial -- a short packet
// may lie inside one word, or straddle two and fill neither -- and are written
// by st_bytes from the lane that holds them: never a load, merge and store of a
// destination word, whose other bytes the neighbouring packet's wave writes in
// this same launch.  The source byte that lands on A0 is src + hs - dlo; its
// low four bits are the shift, uniform per item, and all sixteen occur (k_pack
// sees 6..12), so the word select q = 0..3 is a uniform branch of four and the
// byte shift r goes to v_alignbyte_b32 as a register.  Of the two aligned source
// words around a destination word, one is loaded only if the bytes [b0, b1)
// that the lane owns need a byte of it; those bytes are payload bytes, so
// every load stays inside the aligned words that hold a byte of [src + hs,
// src + hs + n), which k_offsets checked against cap.  Two tiles' loads are in
// flight before their stores.  No LDS, no atomics, no scratch.
__global__ __launch_bounds__(64 * kDeliverWaves) void k_concat(const ConcatJob* __restrict__ jobs,
                                                               const ConcatItem* __restrict__ items,
                                                               const ConcatRec* __restrict__ recs, uint32_t count)
{
    const uint32_t ii = __builtin_amdgcn_readfirstlane(blockIdx.x * kDeliverWaves + (threadIdx.x >> 6));
    if (ii >= count)
        return;
    const uint32_t lane = threadIdx.x & 63;
    const ConcatRec rc = recs[ii];
    if (!(rc.flags & kConcatWrite))   // (uniform)
        return;
    const ConcatItem it = items[ii];
    const uint64_t D = jobs[it.job].dst + rc.off;
    const uint32_t dlo = (uint32_t)(D & 15u);
    const uint64_t A0 = D - dlo;
    const uint64_t total = (uint64_t)dlo + rc.n;          // from A0 to the payload's end
    const uint64_t sbase = it.src + rc.hs - dlo;          // the source byte that lands on A0
    const unsigned sh = (unsigned)(sbase & 15u);          // 0..15
    const unsigned q = sh >> 2, r = sh & 3;
    const uint64_t sa0 = sbase - sh;
    const uint64_t step = (uint64_t)gridDim.y * kIngestChunkBytes;
    for (uint64_t c0 = (uint64_t)blockIdx.y * kIngestChunkBytes; c0 < total; c0 += step) {
        const uint64_t c1 = c0 + kIngestChunkBytes < total ? c0 + kIngestChunkBytes : total;
        for (uint64_t t = c0; t < c1; t += 2 * kTileBytes) {
            uint4 out[2];
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                out[u] = make_uint4(0, 0, 0, 0);
                if (p >= total)
                    continue;
                const uint32_t b0 = p == 0 ? dlo : 0u;
                const uint32_t b1 = total - p < 16 ? (uint32_t)(total - p) : 16u;
                const uint4 lo = sh + b0 < 16 ? ld16(sa0 + p) : make_uint4(0, 0, 0, 0);
                const uint4 hi = sh + b1 > 16 ? ld16(sa0 + p + 16) : make_uint4(0, 0, 0, 0);
                const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                switch (q) {   // wave-uniform
                case 0:
                    out[u] = make_uint4(pick(w, 0, r, 0), pick(w, 0, r, 1), pick(w, 0, r, 2), pick(w, 0, r, 3));
                    break;
                case 1:
                    out[u] = make_uint4(pick(w, 1, r, 0), pick(w, 1, r, 1), pick(w, 1, r, 2), pick(w, 1, r, 3));
                    break;
                case 2:
                    out[u] = make_uint4(pick(w, 2, r, 0), pick(w, 2, r, 1), pick(w, 2, r, 2), pick(w, 2, r, 3));
                    break;
                default:
                    out[u] = make_uint4(pick(w, 3, r, 0), pick(w, 3, r, 1), pick(w, 3, r, 2), pick(w, 3, r, 3));
                    break;
                }
            }
#pragma unroll
            for (unsigned u = 0; u < 2; ++u) {
                const uint64_t p = t + u * kTileBytes + lane * 16;
                if (p >= total)
                    continue;
                const uint32_t b0 = p == 0 ? dlo : 0u;
                const uint32_t b1 = total - p < 16 ? (uint32_t)(total - p) : 16u;
                if (b0 == 0 && b1 == 16)
                    st16(A0 + p, out[u]);
                else
                    st_bytes(A0 + p, out[u], b0, b1);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Row scan (k_scan, ops.h RowHead)
//
// The way in for frame rows that exist only in device memory: one lane per
// row reads the row's first aligned 16 bytes (the header is at most 11), and
// everything the host needs of the row goes out as one 32-byte record, two
// 16-byte stores per lane, 2 KiB contiguous per wave.  The prefix is parsed
// as frames_parse parses it; the header after it is the 128-bit word shifted
// down by the prefix bytes, so type, flow and PacketNum (or a recovery
// packet's first four bytes) are fixed bit fields of one 64-bit value.  A
// recovery row also gives its last min(8, dataBytes) bytes, which end
// anywhere in the row: the one or two aligned words that hold them are loaded
// (the first word again from its register) and recombined with 64-bit shifts
// by the per-lane byte offset.  Both words lie inside the row, because the
// frame ends at or before row + stride and the stride is a multiple of 16.
// Adjacent lanes read addresses `stride` apart, so a wave's load is 64
// requests to 64 different cache lines, not one 1 KiB burst: the kernel is
// bound by request rate, not bytes, and what it buys is that a line or two
// per row is fetched instead of the row.  One lane per row keeps 64
// independent requests in flight per wave; a wave per row would fetch the same
// lines with 63 idle lanes.  No LDS, no atomics.

__device__ __forceinline__ uint64_t pack64(uint32_t lo, uint32_t hi)
{
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kScanThreads) void k_scan(uint64_t rows, uint64_t stride,
                                                       const uint32_t* __restrict__ lens, uint32_t count,
                                                       uint64_t out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    if (k >= count)
        return;
    const uint64_t row = rows + k * stride;
    const uint32_t len = lens ? lens[k] : 0;
    const uint4 f = ld16(row);
    uint4 r0 = make_uint4(0, kRowEmpty, 0, 0), r1 = make_uint4(0, 0, 0, 0);
    if (lens ? len != 0 : (f.x & 0xffu) != 0) {
        r0.y = kRowMalformed;
        uint32_t L = 0;
        const uint32_t h = (uint32_t)parse_prefix(f.x, 4, &L);   // 1..4: four bytes are at hand
        // row bytes [h, h + 8): type, flow, then PacketNum or the packet's first bytes
        const uint64_t x = (pack64(f.x, f.y) >> (8u * h)) | (pack64(f.z, f.w) << (64u - 8u * h));
        const uint32_t type = (uint32_t)x & 0xffu;
        const uint32_t inner = type == 0 ? 7u : 4u;
        const uint32_t flow = (uint32_t)(x >> 8) & 0xffffffu;
        const uint32_t num = type == 0 ? (uint32_t)(x >> 32) & 0xffffffu : 0u;
        const uint32_t total = h + L;   // (L < 2^29)
        if (L >= 1 && (!lens || len == total) && type <= 1 && L > inner && total <= stride && num <= 0x3fffffu &&
            L - inner <= 0x1fffffffu) {
            const uint32_t D = L - inner;
            uint32_t head = 0, T = 0;
            uint64_t tail = 0;
            if (type == 1) {
                head = (uint32_t)(x >> 32) & byte_mask((int)D);
                T = D < 8 ? D : 8;
                const uint32_t s0 = total - T;   // the tail is row bytes [s0, total)
                const uint32_t wlo = s0 & ~15u, whi = (total - 1) & ~15u;   // (whi = wlo or wlo + 16, < stride)
                const uint4 a = wlo == 0 ? f : ld16(row + wlo);
                const uint4 b = whi != wlo ? ld16(row + whi) : make_uint4(0, 0, 0, 0);
                const uint32_t s = s0 & 15u;
                const uint64_t d0 = pack64(a.x, a.y), d1 = pack64(a.z, a.w), d2 = pack64(b.x, b.y);
                const uint64_t A = (s & 8u) ? d1 : d0, B = (s & 8u) ? d2 : d1;
                const uint32_t sh = 8u * (s & 7u);
                uint64_t v = A >> sh;
                if (sh)
                    v |= B << (64u - sh);
                if (T < 8)
                    v &= ((uint64_t)1 << (8u * T)) - 1;
                tail = v << (8u * (8u - T));   // right-aligned
            }
            r0 = make_uint4(total, kRowOk | (type << 8) | ((h + inner) << 16) | (T << 24), flow, num);
            r1 = make_uint4(D, head, (uint32_t)tail, (uint32_t)(tail >> 32));
        }
    }
    st16(out + k * 32, r0);
    st16(out + k * 32 + 16, r1);
}

// ---------------------------------------------------------------------------
// Packed row walk (k_walk, ops.h PackedHead)
//
// k_scan for rows that hold several frames: still one lane per row, but the
// lane walks its row as frames_parse does (frames.h row_walk is the
// statement) and writes one 32-byte record per frame, then zero records up to
// maxFrames and the row word.  The cursor moves through aligned 16-byte
// words: the word that holds it is loaded, the bytes before the cursor and
// at or past the row's end are masked off, and the first non-zero byte that
// is left starts a frame (none: the whole word is skipped, so a zero run costs
// one load per 16 bytes).  A header of up to 11 bytes at byte s of its word
// needs the next word when s > 4; that word is loaded only if it lies inside
// the row, and the 16 bytes from the cursor are the three or four 64-bit
// halves recombined by shifts, after which the fields are k_scan's.  Every
// header byte that is used lies before the row's end, because the prefix is
// judged with the bytes left and the frame must fit; so does the tail, taken
// as in k_scan from the one or two words that hold it.  A frame's walk is a
// chain of dependent loads (the next header's place is known only from this
// one's length), so a lane has one request in flight, and the lanes of a wave
// stay 64 rows apart: the kernel is bound by request latency times frames
// per row, not by bytes.  No LDS, no atomics.

// mask of the low n bytes of a qword, n clamped to [0, 8]
__device__ __forceinline__ uint64_t low_bytes64(int64_t n)
{
    return n <= 0 ? 0ull : (n >= 8 ? ~0ull : (((uint64_t)1 << (8 * n)) - 1));
}

// One row's walk, shared by k_walk and k_walkd: the accepted frames' records
// go to rec, n of them, and the row word n | flags is returned.  Records past
// the n-th are not written here.
__device__ __forceinline__ uint32_t walk_row(uint64_t row, uint64_t stride, uint64_t end, uint32_t maxFrames,
                                             uint64_t rec)
{
    uint32_t n = 0, flags = 0;
    if (end > stride) {
        flags = kPackedMalformed;
        end = 0;
    }
    uint64_t at = 0;
    while (at < end) {
        const uint64_t wa = at & ~(uint64_t)15;
        const uint4 A = ld16(row + wa);
        const uint64_t d0 = pack64(A.x, A.y), d1 = pack64(A.z, A.w);
        // the word's bytes in [at, end)
        const int64_t lo = (int64_t)(at - wa), hi = (int64_t)(end - wa);
        const uint64_t m0 = d0 & low_bytes64(hi) & ~low_bytes64(lo);
        const uint64_t m1 = d1 & low_bytes64(hi - 8) & ~low_bytes64(lo - 8);
        if ((m0 | m1) == 0) {
            at = wa + 16;
            continue;
        }
        const uint32_t s = m0 ? (uint32_t)(__ffsll((long long)m0) - 1) >> 3
                              : 8u + ((uint32_t)(__ffsll((long long)m1) - 1) >> 3);
        at = wa + s;
        if (n == maxFrames) {
            flags |= kPackedMore;
            break;
        }
        // row bytes [at, at + 16), zero where the next word is not loaded
        const uint4 B = (s > 4 && wa + 16 < stride) ? ld16(row + wa + 16) : make_uint4(0, 0, 0, 0);
        const uint64_t d2 = pack64(B.x, B.y), d3 = pack64(B.z, B.w);
        const uint64_t P = (s & 8u) ? d1 : d0, Q = (s & 8u) ? d2 : d1, R = (s & 8u) ? d3 : d2;
        const uint32_t sh = 8u * (s & 7u);
        uint64_t w0 = P >> sh, w1 = Q >> sh;
        if (sh) {
            w0 |= Q << (64u - sh);
            w1 |= R << (64u - sh);
        }
        const uint64_t left = end - at;
        uint32_t L = 0;
        const int hp = parse_prefix((uint32_t)w0, left < 4 ? (uint32_t)left : 4u, &L);
        bool ok = hp >= 1 && L >= 1 && (uint64_t)hp + L <= left;
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = make_uint4(0, 0, 0, 0);
        uint32_t total = 0;
        if (ok) {
            const uint32_t h = (uint32_t)hp;
            // row bytes [at + h, at + h + 8): type, flow, then PacketNum or the packet's first bytes
            const uint64_t x = (w0 >> (8u * h)) | (w1 << (64u - 8u * h));
            const uint32_t type = (uint32_t)x & 0xffu;
            const uint32_t inner = type == 0 ? 7u : 4u;
            const uint32_t flow = (uint32_t)(x >> 8) & 0xffffffu;
            const uint32_t num = type == 0 ? (uint32_t)(x >> 32) & 0xffffffu : 0u;
            total = h + L;   // (L < 2^29)
            ok = type <= 1 && L > inner && num <= 0x3fffffu;
            if (ok) {
                const uint32_t D = L - inner;
                uint32_t head = 0, T = 0;
                uint64_t tail = 0;
                if (type == 1) {
                    head = (uint32_t)(x >> 32) & byte_mask((int)D);
                    T = D < 8 ? D : 8;
                    const uint64_t fe = at + total;   // the tail is row bytes [fe - T, fe), fe <= end
                    const uint64_t s0 = fe - T;
                    const uint64_t wlo = s0 & ~(uint64_t)15, whi = (fe - 1) & ~(uint64_t)15;   // (whi < stride)
                    const uint4 a = wlo == wa ? A : ld16(row + wlo);
                    const uint4 b = whi != wlo ? ld16(row + whi) : make_uint4(0, 0, 0, 0);
                    const uint32_t ts = (uint32_t)s0 & 15u;
                    const uint64_t e0 = pack64(a.x, a.y), e1 = pack64(a.z, a.w), e2 = pack64(b.x, b.y);
                    const uint64_t TA = (ts & 8u) ? e1 : e0, TB = (ts & 8u) ? e2 : e1;
                    const uint32_t tsh = 8u * (ts & 7u);
                    uint64_t v = TA >> tsh;
                    if (tsh)
                        v |= TB << (64u - tsh);
                    if (T < 8)
                        v &= ((uint64_t)1 << (8u * T)) - 1;
                    tail = v << (8u * (8u - T));   // right-aligned
                }
                r0 = make_uint4((uint32_t)at, kRowOk | (type << 8) | ((h + inner) << 16) | (T << 24), flow, num);
                r1 = make_uint4(D, head, (uint32_t)tail, (uint32_t)(tail >> 32));
            }
        }
        if (!ok) {
            flags |= kPackedMalformed;
            break;
        }
        st16(rec + (uint64_t)n * 32, r0);
        st16(rec + (uint64_t)n * 32 + 16, r1);
        ++n;
        at += total;
    }
    return n | flags;
}

__global__ __launch_bounds__(kWalkThreads) void k_walk(uint64_t rows, uint64_t stride,
                                                       const uint32_t* __restrict__ lens, uint32_t count,
                                                       uint32_t maxFrames, uint64_t out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    if (k >= count)
        return;
    const uint64_t rec = out + k * maxFrames * 32;
    const uint32_t word = walk_row(rows + k * stride, stride, lens ? lens[k] : stride, maxFrames, rec);
    for (uint32_t j = word & kPackedCountMask; j < maxFrames; ++j) {   // every record is written by every scan
        st16(rec + (uint64_t)j * 32, make_uint4(0, 0, 0, 0));
        st16(rec + (uint64_t)j * 32 + 16, make_uint4(0, 0, 0, 0));
    }
    *reinterpret_cast<GMEM uint32_t*>(out + (uint64_t)count * maxFrames * 32 + k * 4) = word;
}

// ---------------------------------------------------------------------------
// Dense packed scan (k_walkd, k_rowsum, k_compact; ops.h dense_bytes,
// frames.h dense_compact is the statement)
//
// k_walk's records without the slots no frame filled: the walk writes each
// row's records into a scratch area that stays on the device, a prefix sum over
// the rows' counts places them, and a copy packs them back to back, so the bytes
// that cross to the host follow the frames there are and not count * maxFrames.

// k_walkd: k_walk's lane per row and walk_row, the records into the row's
// maxFrames scratch slots (those past the n-th stay unwritten: k_compact reads
// none of them) and the row word into the output's word table.
__global__ __launch_bounds__(kWalkThreads) void k_walkd(uint64_t rows, uint64_t stride,
                                                        const uint32_t* __restrict__ lens, uint32_t count,
                                                        uint32_t maxFrames, uint64_t scratch, uint64_t words)
{
    const uint64_t k = (uint64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    if (k >= count)
        return;
    *reinterpret_cast<GMEM uint32_t*>(words + k * 4) =
        walk_row(rows + k * stride, stride, lens ? lens[k] : stride, maxFrames, scratch + k * maxFrames * 32);
}

// inclusive sum of v over the lanes of a wave up to this one (six __shfl_up
// steps: k_offsets' scan on 32-bit values, which the rows' counts fit)
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (unsigned s = 1; s < 64; s <<= 1) {
        const uint32_t u = __shfl_up(v, s);
        if (lane >= s)
            v += u;
    }
    return v;
}

// k_rowsum: start[] = the exclusive prefix sum of the rows' counts, and from it
// c, W, T, the info words and the zero padding before the records.  The carry
// scheme is a single workgroup striding over the rows: kRowsumThreads lanes,
// lane t of a pass owning the kRowsumRows consecutive rows from base + t *
// kRowsumRows, so a pass covers kRowsumPass rows and the running sum of the
// passes before is a register that every lane holds.  Within a pass a lane sums
// its rows, the wave scans the lane sums (wave_incl_sum), lane 63 of each wave
// leaves the wave's sum in LDS and, after one barrier, every lane adds the sums
// of the waves before its own.  The table of wave sums is double-buffered by the
// pass's parity, so one barrier per pass is enough: a wave that writes pass
// p + 2's sums has passed pass p + 1's barrier, which no wave reaches before it
// has read pass p's.  This was chosen over a two-level block-sum pass because it
// is one launch without a second kernel or a grid-wide wait, its order of
// additions is fixed by the row index alone, and it is short beside the walk: 40
// passes for 327,680 rows, with the next pass's words loaded (two 16-byte loads
// per lane) before this pass's scan so that their latency is hidden.  A count
// above maxFrames, which the walk never writes, is clamped, so a row's span in
// the scratch area can never be left.  Rows are complete while start[k + 1] <=
// maxRecords; the starts only grow, so the number of such rows is c and the
// largest such start is W: both are reduced over the workgroup through LDS,
// integers in a fixed order.  No atomics.
__global__ __launch_bounds__(kRowsumThreads) void k_rowsum(uint64_t out, uint32_t count, uint32_t maxFrames,
                                                           uint32_t maxRecords)
{
    constexpr uint32_t kWaves = kRowsumThreads / 64;
    __shared__ uint32_t wsum[2][kWaves];
    __shared__ uint32_t redC[kWaves], redW[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t words = out + 16, starts = words + (uint64_t)count * 4;
    auto load = [&](uint32_t base, uint32_t* n) {
        const uint64_t r0 = (uint64_t)base + tid * kRowsumRows;
        if (r0 + kRowsumRows <= count) {   // (16-byte aligned: base and kRowsumRows are multiples of 4)
            const uint4 a = ld16(words + r0 * 4), b = ld16(words + r0 * 4 + 16);
            n[0] = a.x, n[1] = a.y, n[2] = a.z, n[3] = a.w;
            n[4] = b.x, n[5] = b.y, n[6] = b.z, n[7] = b.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kRowsumRows; ++j)
                n[j] = r0 + j < count ? *reinterpret_cast<const GMEM uint32_t*>(words + (r0 + j) * 4) : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < kRowsumRows; ++j) {
            n[j] &= kPackedCountMask;
            n[j] = n[j] < maxFrames ? n[j] : maxFrames;
        }
    };
    static_assert(kRowsumRows == 8, "k_rowsum loads a lane's rows as two 16-byte words");
    uint32_t carry = 0, done = 0, W = 0;
    uint32_t nx[kRowsumRows];
    load(0, nx);
    for (uint32_t base = 0, p = 0; base < count; base += kRowsumPass, p ^= 1) {
        uint32_t n[kRowsumRows];
        uint32_t s = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRowsumRows; ++j) {
            n[j] = nx[j];
            s += n[j];
        }
        if (count - base > kRowsumPass)
            load(base + kRowsumPass, nx);
        const uint32_t incl = wave_incl_sum(s, lane);
        if (lane == 63)
            wsum[p][wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t v = wsum[p][w];
            total += v;
            before += w < wave ? v : 0u;
        }
        uint32_t at = carry + before + incl - s;
        const uint64_t r0 = (uint64_t)base + tid * kRowsumRows;
#pragma unroll
        for (uint32_t j = 0; j < kRowsumRows; ++j) {
            if (r0 + j < count) {
                *reinterpret_cast<GMEM uint32_t*>(starts + (r0 + j) * 4) = at;
                at += n[j];
                if (at <= maxRecords) {
                    ++done;
                    W = at;
                }
            }
        }
        carry += total;
    }
    // c = the sum of done, W = the largest W (0 where no row is complete)
#pragma unroll
    for (unsigned s = 32; s >= 1; s >>= 1) {
        done += __shfl_xor(done, s);
        const uint32_t o = __shfl_xor(W, s);
        W = W > o ? W : o;
    }
    if (lane == 0) {
        redC[wave] = done;
        redW[wave] = W;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0, w = 0;
        for (uint32_t i = 0; i < kWaves; ++i) {
            c += redC[i];
            w = w > redW[i] ? w : redW[i];
        }
        *reinterpret_cast<GMEM uint32_t*>(starts + (uint64_t)count * 4) = carry;
        for (uint64_t a = starts + (uint64_t)(count + 1) * 4; a < out + dense_records_offset(count); a += 4)
            *reinterpret_cast<GMEM uint32_t*>(a) = 0;
        st16(out, make_uint4(carry, w, c, 0));
    }
}

// k_compact: one record slot of the output per pair of lanes, each lane one
// 16-byte half, over all maxRecords slots: a wave stores 1 KiB of consecutive
// bytes.  Slot i < W belongs to the row k with start[k] <= i < start[k + 1]
// (rows without frames share a start with the next row and own no slot): a
// binary search over start[0, c], whose two ends hold 0 and W, so k < c always;
// the table is count + 1 words that every lane reads and stays in cache.  The
// slot is record i - start[k] of row k's scratch span (below maxFrames, by
// k_rowsum's clamp); a slot from W on is zero.  No LDS, no atomics.
__global__ __launch_bounds__(kCompactThreads) void k_compact(uint64_t out, uint64_t scratch, uint32_t count,
                                                             uint32_t maxFrames, uint32_t maxRecords)
{
    const uint64_t g = (uint64_t)blockIdx.x * kCompactThreads + threadIdx.x;
    const uint64_t i = g >> 1;
    if (i >= maxRecords)
        return;
    const uint64_t half = (g & 1) * 16;
    const uint4 info = ld16(out);   // {T, W, c, 0 or the dense duplex scan's WA, which is not read here}
    const uint32_t c = info.z < count ? info.z : count;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i < info.y && c != 0) {
        const uint64_t starts = out + 16 + (uint64_t)count * 4;
        uint32_t lo = 0, hi = c;   // start[lo] <= i < start[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (*reinterpret_cast<const GMEM uint32_t*>(starts + (uint64_t)mid * 4) <= i)
                lo = mid;
            else
                hi = mid;
        }
        const uint64_t j = i - *reinterpret_cast<const GMEM uint32_t*>(starts + (uint64_t)lo * 4);
        if (j < maxFrames)
            v = ld16(scratch + ((uint64_t)lo * maxFrames + j) * 32 + half);
    }
    st16(out + dense_records_offset(count) + i * 32 + half, v);
}

// ---------------------------------------------------------------------------
// Stream row walk (k_streamwalk, ops.h kStreamPartial; frames.h stream_walk is
// the statement)
//
// The dense scan for rows that are byte streams: row bytes [start, end) hold
// frames back to back and the last one may be cut off by end.  walk_row's lane
// per row is bound by a chain of dependent loads, one frame at a time; here a
// wave takes the row, kStreamChunk bytes at a time, and the chain is followed
// in LDS.  A chunk starts at the 16-byte word that holds the cursor: lane l
// loads word l, lane 0 also the word behind the chunk (a header of up to 11
// bytes that starts in the chunk's last bytes ends there), words at or past the
// stride read as zero.  Every lane then judges, for its 16 byte positions, the
// frame that would start there (stream_hop: walk_row's rules plus the partial
// rule) and leaves the hop in LDS: the next position after a zero byte, the
// position behind an accepted frame, or kStreamChunk for every hop that leaves
// the chunk or stops the walk.  The positions the walk really visits are the
// chain from the cursor; it is found by pointer doubling: in round r every
// reached position marks the one 2^r hops behind it and hands it its rank (the
// frames before it), then every position squares its hop.  A round that marks
// nothing ends the search, so a chunk of a few long frames takes two or three
// rounds and only a chunk of zero bytes takes all ten.  The lanes that own
// reached frames then build their records from the staged bytes and store them
// at slot n + rank of the row's scratch slots; a recovery frame's tail is one
// or two global loads per lane, independent of every other lane's, so the tail
// loads of a chunk's frames are in flight together.  The wave carries the
// cursor, the count and the flags into the next chunk, which starts where the
// last hop landed: the chunks inside a long frame are never loaded.  A wave's
// LDS accesses are executed in order, so what one lane wrote is there for
// another lane's later read; wave_lds_sync only keeps the compiler from moving
// accesses across the hand-over.  No workgroup barrier (the waves of a
// workgroup share nothing), no atomics.  k_rowsum masks the row word with
// kPackedCountMask before it sums, so kStreamPartial rides along in the word as
// kPackedMore and kPackedMalformed do, and k_compact reads only the starts: both
// run unchanged behind this walk.

constexpr uint32_t kStreamWaves = kStreamWalkThreads / 64;
constexpr uint32_t kStreamPer = kStreamChunk / 64;   // byte positions per lane
constexpr uint32_t kStreamNone = 0xffffu;            // rank of a position the chain has not reached
static_assert(kStreamChunk == 64 * 16 && kStreamChunk < kStreamNone, "a chunk is one 16-byte word per lane");

// what the walk does at a byte position
enum : uint32_t
{
    kHopZero,      // a zero byte: on to the next position
    kHopFrame,     // an accepted frame: on to the position behind it
    kHopExit,      // (of a chunk's last position only: the hop leaves the chunk)
    kHopEnd,       // the row's bytes are used up
    kHopPartial,   // a frame the data does not yet hold whole
    kHopBad        // a frame that is malformed, or cut off and never valid
};
struct StreamHop
{
    uint32_t kind, h, L;
    uint64_t x;   // row bytes [a + h, a + h + 8): type, flow, then PacketNum or the packet's first bytes
};

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The frame that would start at row offset a < end, from row bytes [a, a + 12)
// (y0..y2; only those before end are used).
__device__ __forceinline__ StreamHop stream_hop(uint32_t y0, uint32_t y1, uint32_t y2, uint64_t a, uint64_t end,
                                                uint64_t stride)
{
    StreamHop r = {kHopZero, 0, 0, 0};
    if ((y0 & 0xffu) == 0)
        return r;
    const uint64_t left = end - a;
    uint32_t L = 0;
    const int hp = parse_prefix(y0, left < 4 ? (uint32_t)left : 4u, &L);
    if (hp < 1) {   // the prefix itself is cut off
        r.kind = kHopPartial;
        return r;
    }
    if (L < 1) {
        r.kind = kHopBad;
        return r;
    }
    const uint32_t h = (uint32_t)hp;
    const uint64_t x = (pack64(y0, y1) >> (8u * h)) | ((uint64_t)y2 << (64u - 8u * h));
    const uint32_t type = (uint32_t)x & 0xffu;
    const uint32_t inner = type == 0 ? 7u : 4u;
    const uint32_t num = type == 0 ? (uint32_t)(x >> 32) & 0xffffffu : 0u;
    r.h = h;
    r.L = L;
    r.x = x;
    if ((uint64_t)h + L <= left) {
        r.kind = type <= 1 && L > inner && num <= 0x3fffffu ? kHopFrame : kHopBad;
        return r;
    }
    const uint64_t have = left - h;   // bytes of the frame's body that are there
    bool never = (uint64_t)h + L > stride;
    if (have >= 1)
        never = never || type > 1 || L <= inner;
    if (have >= 7)
        never = never || num > 0x3fffffu;
    r.kind = never ? kHopBad : kHopPartial;
    return r;
}

__global__ __launch_bounds__(kStreamWalkThreads) void k_streamwalk(uint64_t rows, uint64_t stride,
                                                                   const uint32_t* __restrict__ starts,
                                                                   const uint32_t* __restrict__ ends, uint32_t count,
                                                                   uint32_t maxFrames, uint64_t scratch,
                                                                   uint64_t words, uint64_t nexts)
{
    constexpr uint32_t C = kStreamChunk;
    __shared__ uint4 sBytes[kStreamWaves][C / 16 + 1];
    __shared__ uint16_t sJmp[kStreamWaves][C], sCnt[kStreamWaves][C], sRank[kStreamWaves][C];
    __shared__ uint32_t sLast[kStreamWaves][4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t k = (uint64_t)blockIdx.x * kStreamWaves + wave;
    if (k >= count)   // (wave-uniform)
        return;
    const uint32_t* B = reinterpret_cast<const uint32_t*>(sBytes[wave]);
    uint16_t* jmp = sJmp[wave];
    uint16_t* cnt = sCnt[wave];
    uint16_t* rank = sRank[wave];
    uint32_t* last = sLast[wave];
    const uint64_t row = rows + k * stride;
    const uint64_t start = starts ? starts[k] : 0, end = ends ? ends[k] : stride;
    const uint64_t rec = scratch + k * maxFrames * 32;
    // row bytes [base + p, base + p + 12) of the staged chunk
    auto bytes12 = [&](uint32_t p, uint32_t& y0, uint32_t& y1, uint32_t& y2) {
        const uint32_t q = p >> 2, s = p & 3u;
        const uint32_t x0 = B[q], x1 = B[q + 1], x2 = B[q + 2], x3 = B[q + 3];
        y0 = __builtin_amdgcn_alignbyte(x1, x0, s);
        y1 = __builtin_amdgcn_alignbyte(x2, x1, s);
        y2 = __builtin_amdgcn_alignbyte(x3, x2, s);
    };
    uint32_t n = 0, flags = 0;
    uint64_t at = start, next = end;
    bool open = true;
    if (start > end || end > stride) {
        flags = kPackedMalformed;
        next = start < stride ? start : stride;
        open = false;
    }
    while (open && at < end) {   // (all wave-uniform)
        const uint64_t base = at & ~(uint64_t)15;
        const uint32_t entry = (uint32_t)(at - base);
        // 1. stage the chunk and its halo
        {
            const uint64_t a = base + lane * 16;
            sBytes[wave][lane] = a < stride ? ld16(row + a) : make_uint4(0, 0, 0, 0);
            if (lane == 0) {
                sBytes[wave][C / 16] = base + C < stride ? ld16(row + base + C) : make_uint4(0, 0, 0, 0);
                // (step 4 overwrites this with the chain's last position: a chunk can only end the walk or
                // move the cursor on, whatever the chain turns out to be)
                last[0] = kHopBad;
                last[1] = 0;
                last[2] = (uint32_t)at;
                last[3] = (uint32_t)(at >> 32);
            }
        }
        wave_lds_sync();
        // 2. every position's hop
#pragma unroll
        for (uint32_t i = 0; i < kStreamPer; ++i) {
            const uint32_t p = i * 64 + lane;
            const uint64_t a = base + p;
            uint32_t j = C, c = 0;
            if (a < end) {
                uint32_t y0, y1, y2;
                bytes12(p, y0, y1, y2);
                const StreamHop hop = stream_hop(y0, y1, y2, a, end, stride);
                if (hop.kind == kHopZero) {
                    j = p + 1;
                } else if (hop.kind == kHopFrame) {
                    const uint32_t t = p + hop.h + hop.L;   // (L < 2^29)
                    j = t < C ? t : C;
                    c = 1;
                }
            }
            jmp[p] = (uint16_t)j;
            cnt[p] = (uint16_t)c;
            rank[p] = (uint16_t)(p == entry ? 0u : kStreamNone);
        }
        wave_lds_sync();
        // 3. the chain from the entry, by pointer doubling
        for (;;) {
            uint32_t r[kStreamPer], j[kStreamPer], c[kStreamPer], jj[kStreamPer], cc[kStreamPer];
#pragma unroll
            for (uint32_t i = 0; i < kStreamPer; ++i) {
                const uint32_t p = i * 64 + lane;
                r[i] = rank[p];
                j[i] = jmp[p];
                c[i] = cnt[p];
                jj[i] = j[i] < C ? jmp[j[i]] : C;
                cc[i] = j[i] < C ? cnt[j[i]] : 0u;
            }
            wave_lds_sync();
            bool marked = false;
#pragma unroll
            for (uint32_t i = 0; i < kStreamPer; ++i) {
                const uint32_t p = i * 64 + lane;
                if (r[i] != kStreamNone && j[i] < C) {   // (one reached position at most hops to j)
                    rank[j[i]] = (uint16_t)(r[i] + c[i]);
                    marked = true;
                }
                jmp[p] = (uint16_t)jj[i];
                cnt[p] = (uint16_t)(c[i] + cc[i]);
            }
            wave_lds_sync();
            if (!__any(marked))
                break;
        }
        // 4. the reached frames' records; the chain's last position says how the chunk ends
        const uint32_t room = maxFrames - n;
        uint32_t morePos = C;   // the first reached non-zero byte with `room` frames before it
#pragma unroll
        for (uint32_t i = 0; i < kStreamPer; ++i) {
            const uint32_t p = i * 64 + lane;
            const uint64_t a = base + p;
            const uint32_t r = rank[p];
            if (r == kStreamNone)
                continue;
            uint32_t kind = kHopEnd, frames = r;
            uint64_t pos = a;
            bool isLast = true;
            if (a < end) {
                uint32_t y0, y1, y2;
                bytes12(p, y0, y1, y2);
                const StreamHop hop = stream_hop(y0, y1, y2, a, end, stride);
                kind = hop.kind;
                if (kind == kHopZero) {
                    isLast = p + 1 == C;
                    kind = kHopExit;
                    pos = a + 1;
                } else if (r >= room) {
                    morePos = p < morePos ? p : morePos;
                    isLast = false;
                } else if (kind == kHopFrame) {
                    const uint32_t h = hop.h, L = hop.L, total = h + L;
                    const uint64_t x = hop.x;
                    const uint32_t type = (uint32_t)x & 0xffu;
                    const uint32_t inner = type == 0 ? 7u : 4u;
                    const uint32_t flow = (uint32_t)(x >> 8) & 0xffffffu;
                    const uint32_t num = type == 0 ? (uint32_t)(x >> 32) & 0xffffffu : 0u;
                    const uint32_t D = L - inner;
                    uint32_t head = 0, T = 0;
                    uint64_t tail = 0;
                    if (type == 1) {
                        head = (uint32_t)(x >> 32) & byte_mask((int)D);
                        T = D < 8 ? D : 8;
                        const uint64_t fe = a + total;   // the tail is row bytes [fe - T, fe), fe <= end
                        const uint64_t s0 = fe - T;
                        const uint64_t wlo = s0 & ~(uint64_t)15, whi = (fe - 1) & ~(uint64_t)15;   // (whi < stride)
                        const uint4 ta = ld16(row + wlo);
                        const uint4 tb = whi != wlo ? ld16(row + whi) : make_uint4(0, 0, 0, 0);
                        const uint32_t ts = (uint32_t)s0 & 15u;
                        const uint64_t e0 = pack64(ta.x, ta.y), e1 = pack64(ta.z, ta.w), e2 = pack64(tb.x, tb.y);
                        const uint64_t TA = (ts & 8u) ? e1 : e0, TB = (ts & 8u) ? e2 : e1;
                        const uint32_t tsh = 8u * (ts & 7u);
                        uint64_t v = TA >> tsh;
                        if (tsh)
                            v |= TB << (64u - tsh);
                        if (T < 8)
                            v &= ((uint64_t)1 << (8u * T)) - 1;
                        tail = v << (8u * (8u - T));   // right-aligned
                    }
                    const uint64_t slot = rec + (uint64_t)(n + r) * 32;   // (n + r < maxFrames)
                    st16(slot, make_uint4((uint32_t)a, kRowOk | (type << 8) | ((h + inner) << 16) | (T << 24), flow,
                                          num));
                    st16(slot + 16, make_uint4(D, head, (uint32_t)tail, (uint32_t)(tail >> 32)));
                    frames = r + 1;
                    isLast = p + total >= C;
                    kind = kHopExit;
                    pos = a + total;
                }
            }
            if (isLast) {
                last[0] = kind;
                last[1] = frames;
                last[2] = (uint32_t)pos;
                last[3] = (uint32_t)(pos >> 32);
            }
        }
        wave_lds_sync();
#pragma unroll
        for (unsigned s = 32; s >= 1; s >>= 1) {
            const uint32_t o = __shfl_xor(morePos, s);
            morePos = o < morePos ? o : morePos;
        }
        if (morePos < C) {   // (the frames of rank below room were all stored)
            n = maxFrames;
            flags |= kPackedMore;
            next = base + morePos;
            open = false;
        } else {
            const uint32_t kind = last[0];
            const uint64_t pos = pack64(last[2], last[3]);
            n += last[1];
            if (kind == kHopExit) {
                at = pos;
            } else {
                flags |= kind == kHopPartial ? kStreamPartial : kind == kHopBad ? kPackedMalformed : 0u;
                next = kind == kHopEnd ? end : pos;
                open = false;
            }
        }
        wave_lds_sync();   // (the next chunk's stage overwrites what was read here)
    }
    if (lane == 0) {
        *reinterpret_cast<GMEM uint32_t*>(words + k * 4) = n | flags;
        *reinterpret_cast<GMEM uint32_t*>(nexts + k * 4) = next < 0xffffffffull ? (uint32_t)next : 0xffffffffu;
    }
    // the zeros between the next words and the next 16-byte boundary: every byte is written by every scan
    if (k == (uint64_t)count - 1 && lane >= 1 && lane < 4 && k + lane < (((uint64_t)count + 3) & ~(uint64_t)3))
        *reinterpret_cast<GMEM uint32_t*>(nexts + (k + lane) * 4) = 0;
}

// ---------------------------------------------------------------------------
// Duplex row walk (k_ackwalk, ops.h kRowTruncated)
//
// k_walk for the rows of a bidirectional flow (frames.h ack_walk is the
// statement): the same lane per row and the same cursor, with frames of type
// 2 accepted.  Their record needs no tail; what the host needs is the whole
// acknowledgement message, which goes into the row's next message slot behind
// the row words.  The message starts at any byte of the row and the slot is
// 16-byte aligned, so the lane streams it: each aligned word of the row is
// loaded once, the 16 bytes from the message's cursor are the shifted halves of
// two neighbouring words (k_walk's recombination), the last word is masked to
// the message's end, and the slot is written in whole 16-byte stores, zeros to
// its end.  A word is loaded only when a message byte lies in it, and the
// message ends at or before the row's end: nothing past the row is read.  All
// output goes to the scan's device staging area and crosses to the host in one
// copy, so no lane ever stores bytes into host memory.  A message longer than
// its slot, or an ack after the row's last slot, is reported as truncated and
// the walk goes on behind it.  No LDS, no atomics.

// One row's duplex walk, shared by k_ackwalk and k_ackwalkd: the accepted
// frames' records go to rec, n of them, each ack's message into the next of the
// row's slots from slot0 on (a used slot is written whole, zeros to its end),
// *acksOut = the ack frames accepted and the row word n | flags is returned.
// Records past the n-th and slots past the last used one are not written here.
//
// kStream (k_ackstreamwalk; frames.h ack_stream_walk is the statement): the row
// is a byte stream, walked over [start, end), and *nextOut = where its next scan
// starts.  The cursor starts at `start`, so the first word's mask drops the
// bytes before it as it drops those from `end` on in the last: stale bytes on
// either side never reach a decision.  A frame that the left = end - at bytes
// do not hold whole is classified from its header bytes below end alone (have =
// left - h of them): the 16 bytes recombined at the cursor may hold stale bytes
// behind end, or zeros where the word behind the row's last was not loaded, and
// neither is looked at.  Without kStream, start and nextOut are unused and the
// code is what k_ackwalk and k_ackwalkd have always run.
template <bool kStream>
__device__ __forceinline__ uint32_t ackwalk_row(uint64_t row, uint64_t stride, uint64_t start, uint64_t end,
                                                uint32_t maxFrames, uint32_t ackSlots, uint32_t ackBytes,
                                                uint64_t rec, uint64_t slot0, uint32_t* acksOut, uint64_t* nextOut)
{
    uint32_t n = 0, acks = 0, flags = 0;
    uint64_t at = 0;
    uint64_t stop = end;   // (kStream: where the next scan starts; `end` when only zero bytes are left)
    if constexpr (kStream) {
        if (start > end || end > stride) {
            flags = kPackedMalformed;
            stop = start < stride ? start : stride;
            end = 0;
        } else {
            at = start;
        }
    } else {
        if (end > stride) {
            flags = kPackedMalformed;
            end = 0;
        }
    }
    while (at < end) {
        const uint64_t wa = at & ~(uint64_t)15;
        const uint4 A = ld16(row + wa);
        const uint64_t d0 = pack64(A.x, A.y), d1 = pack64(A.z, A.w);
        // the word's bytes in [at, end)
        const int64_t lo = (int64_t)(at - wa), hi = (int64_t)(end - wa);
        const uint64_t m0 = d0 & low_bytes64(hi) & ~low_bytes64(lo);
        const uint64_t m1 = d1 & low_bytes64(hi - 8) & ~low_bytes64(lo - 8);
        if ((m0 | m1) == 0) {
            at = wa + 16;
            continue;
        }
        const uint32_t s = m0 ? (uint32_t)(__ffsll((long long)m0) - 1) >> 3
                              : 8u + ((uint32_t)(__ffsll((long long)m1) - 1) >> 3);
        at = wa + s;
        if (n == maxFrames) {
            flags |= kPackedMore;
            stop = at;
            break;
        }
        // row bytes [at, at + 16), zero where the next word is not loaded
        const uint4 B = (s > 4 && wa + 16 < stride) ? ld16(row + wa + 16) : make_uint4(0, 0, 0, 0);
        const uint64_t d2 = pack64(B.x, B.y), d3 = pack64(B.z, B.w);
        const uint64_t P = (s & 8u) ? d1 : d0, Q = (s & 8u) ? d2 : d1, R = (s & 8u) ? d3 : d2;
        const uint32_t sh = 8u * (s & 7u);
        uint64_t w0 = P >> sh, w1 = Q >> sh;
        if (sh) {
            w0 |= Q << (64u - sh);
            w1 |= R << (64u - sh);
        }
        const uint64_t left = end - at;
        uint32_t L = 0;
        const int hp = parse_prefix((uint32_t)w0, left < 4 ? (uint32_t)left : 4u, &L);
        bool ok = hp >= 1 && L >= 1 && (uint64_t)hp + L <= left;
        if constexpr (kStream) {
            if (!ok) {   // not whole: partial, unless what is there can never become a valid frame
                bool never = hp >= 1 && L < 1;
                if (hp >= 1 && L >= 1) {
                    const uint32_t h = (uint32_t)hp;
                    const uint64_t have = left - h;   // header bytes behind the prefix that lie below end
                    const uint64_t x = (w0 >> (8u * h)) | (w1 << (64u - 8u * h));
                    const uint32_t type = (uint32_t)x & 0xffu;
                    const uint32_t inner = type == 0 ? 7u : 4u;
                    const uint32_t num = type == 0 ? (uint32_t)(x >> 32) & 0xffffffu : 0u;
                    never = (uint64_t)h + L > stride;
                    if (have >= 1)
                        never = never || type > 2 || L <= inner;
                    if (have >= 7)
                        never = never || num > 0x3fffffu;
                }
                flags |= never ? kPackedMalformed : kStreamPartialDuplex;
                stop = at;
                break;
            }
        }
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = make_uint4(0, 0, 0, 0);
        uint32_t total = 0;
        if (ok) {
            const uint32_t h = (uint32_t)hp;
            // row bytes [at + h, at + h + 8): type, flow, then PacketNum or the packet's first bytes
            const uint64_t x = (w0 >> (8u * h)) | (w1 << (64u - 8u * h));
            const uint32_t type = (uint32_t)x & 0xffu;
            const uint32_t inner = type == 0 ? 7u : 4u;
            const uint32_t flow = (uint32_t)(x >> 8) & 0xffffffu;
            const uint32_t num = type == 0 ? (uint32_t)(x >> 32) & 0xffffffu : 0u;
            total = h + L;   // (L < 2^29)
            ok = type <= 2 && L > inner && num <= 0x3fffffu;
            if (ok && type == 2) {
                const uint32_t D = L - inner;
                uint32_t status = kRowOk;
                if (acks >= ackSlots || D > ackBytes) {
                    status = kRowTruncated;
                    flags |= kPackedAcksDropped;
                }
                if (acks < ackSlots) {
                    // the message is row bytes [p0, fe), fe <= end <= stride; the slot takes [p0, p0 + copy)
                    const uint32_t copy = D < ackBytes ? D : ackBytes;
                    const uint64_t p0 = at + h + inner, fe = p0 + copy;
                    const uint64_t slot = slot0 + (uint64_t)acks * ackBytes;
                    const uint32_t ms = (uint32_t)p0 & 15u, msh = 8u * (ms & 7u);
                    uint64_t mw = p0 & ~(uint64_t)15;
                    uint4 C = mw == wa ? A : ld16(row + mw);   // (mw < fe <= stride)
                    for (uint32_t o = 0; o < ackBytes; o += 16) {
                        uint4 v = make_uint4(0, 0, 0, 0);
                        if (o < copy) {
                            // the next word only when a message byte lies in it (then mw + 16 < fe <= stride)
                            const uint4 N = mw + 16 < fe ? ld16(row + mw + 16) : make_uint4(0, 0, 0, 0);
                            const uint64_t c0 = pack64(C.x, C.y), c1 = pack64(C.z, C.w);
                            const uint64_t c2 = pack64(N.x, N.y), c3 = pack64(N.z, N.w);
                            const uint64_t MP = (ms & 8u) ? c1 : c0, MQ = (ms & 8u) ? c2 : c1, MR = (ms & 8u) ? c3 : c2;
                            uint64_t v0 = MP >> msh, v1 = MQ >> msh;
                            if (msh) {
                                v0 |= MQ << (64u - msh);
                                v1 |= MR << (64u - msh);
                            }
                            const int64_t rem = (int64_t)copy - (int64_t)o;
                            v0 &= low_bytes64(rem);
                            v1 &= low_bytes64(rem - 8);
                            v = make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32));
                            C = N;
                            mw += 16;
                        }
                        st16(slot + o, v);
                    }
                }
                r0 = make_uint4((uint32_t)at, status | (type << 8) | ((h + inner) << 16), flow, acks);
                r1 = make_uint4(D, 0, 0, 0);
                ++acks;
            } else if (ok) {
                const uint32_t D = L - inner;
                uint32_t head = 0, T = 0;
                uint64_t tail = 0;
                if (type == 1) {
                    head = (uint32_t)(x >> 32) & byte_mask((int)D);
                    T = D < 8 ? D : 8;
                    const uint64_t fe = at + total;   // the tail is row bytes [fe - T, fe), fe <= end
                    const uint64_t s0 = fe - T;
                    const uint64_t wlo = s0 & ~(uint64_t)15, whi = (fe - 1) & ~(uint64_t)15;   // (whi < stride)
                    const uint4 a = wlo == wa ? A : ld16(row + wlo);
                    const uint4 b = whi != wlo ? ld16(row + whi) : make_uint4(0, 0, 0, 0);
                    const uint32_t ts = (uint32_t)s0 & 15u;
                    const uint64_t e0 = pack64(a.x, a.y), e1 = pack64(a.z, a.w), e2 = pack64(b.x, b.y);
                    const uint64_t TA = (ts & 8u) ? e1 : e0, TB = (ts & 8u) ? e2 : e1;
                    const uint32_t tsh = 8u * (ts & 7u);
                    uint64_t v = TA >> tsh;
                    if (tsh)
                        v |= TB << (64u - tsh);
                    if (T < 8)
                        v &= ((uint64_t)1 << (8u * T)) - 1;
                    tail = v << (8u * (8u - T));   // right-aligned
                }
                r0 = make_uint4((uint32_t)at, kRowOk | (type << 8) | ((h + inner) << 16) | (T << 24), flow, num);
                r1 = make_uint4(D, head, (uint32_t)tail, (uint32_t)(tail >> 32));
            }
        }
        if (!ok) {
            flags |= kPackedMalformed;
            stop = at;
            break;
        }
        st16(rec + (uint64_t)n * 32, r0);
        st16(rec + (uint64_t)n * 32 + 16, r1);
        ++n;
        at += total;
    }
    if constexpr (kStream)
        *nextOut = stop;
    *acksOut = acks;
    return n | flags;
}

__global__ __launch_bounds__(kAckWalkThreads) void k_ackwalk(uint64_t rows, uint64_t stride,
                                                             const uint32_t* __restrict__ lens, uint32_t count,
                                                             uint32_t maxFrames, uint32_t ackSlots,
                                                             uint32_t ackBytes, uint64_t out, uint64_t slots)
{
    const uint64_t k = (uint64_t)blockIdx.x * kAckWalkThreads + threadIdx.x;
    if (k >= count)
        return;
    const uint64_t rec = out + k * maxFrames * 32;
    const uint64_t slot0 = slots + k * ackSlots * ackBytes;
    uint32_t acks = 0;
    const uint32_t word = ackwalk_row<false>(rows + k * stride, stride, 0, lens ? lens[k] : stride, maxFrames,
                                             ackSlots, ackBytes, rec, slot0, &acks, nullptr);
    for (uint32_t j = word & kPackedCountMask; j < maxFrames; ++j) {   // every record is written by every scan
        st16(rec + (uint64_t)j * 32, make_uint4(0, 0, 0, 0));
        st16(rec + (uint64_t)j * 32 + 16, make_uint4(0, 0, 0, 0));
    }
    for (uint32_t a = acks; a < ackSlots; ++a)   // and every slot
        for (uint32_t o = 0; o < ackBytes; o += 16)
            st16(slot0 + (uint64_t)a * ackBytes + o, make_uint4(0, 0, 0, 0));
    *reinterpret_cast<GMEM uint32_t*>(out + (uint64_t)count * maxFrames * 32 + k * 4) = word;
    if (k + 1 == count)   // the words between the last row word and the first slot
        for (uint64_t p = out + (uint64_t)count * maxFrames * 32 + (uint64_t)count * 4; p < slots; p += 4)
            *reinterpret_cast<GMEM uint32_t*>(p) = 0;
}

// ---------------------------------------------------------------------------
// Dense duplex scan (k_ackwalkd, k_rowsum2, k_compact, k_slots; ops.h
// duplex_dense_bytes, frames.h duplex_dense_compact is the statement)
//
// The dense scan's scheme with the acks' slots as a second compacted list: the
// walk writes each row's records, slots and ack count into scratch areas that
// stay on the device, one prefix sum over both counts places them and decides
// which rows are complete under both budgets, k_compact (unchanged) packs the
// records and k_slots the slots.

// k_ackwalkd: k_ackwalk's lane per row and ackwalk_row, the records into the
// row's maxFrames scratch record slots, the messages into its ackSlots scratch
// message slots (records past the n-th and slots past the last used one stay
// unwritten: k_compact and k_slots read none of them), the row word into the
// output's word table and min(acks, ackSlots) into the scratch count table.
__global__ __launch_bounds__(kAckWalkdThreads) void k_ackwalkd(uint64_t rows, uint64_t stride,
                                                               const uint32_t* __restrict__ lens, uint32_t count,
                                                               uint32_t maxFrames, uint32_t ackSlots,
                                                               uint32_t ackBytes, uint64_t scratchRecs,
                                                               uint64_t scratchSlots, uint64_t scratchCounts,
                                                               uint64_t words)
{
    const uint64_t k = (uint64_t)blockIdx.x * kAckWalkdThreads + threadIdx.x;
    if (k >= count)
        return;
    uint32_t acks = 0;
    *reinterpret_cast<GMEM uint32_t*>(words + k * 4) =
        ackwalk_row<false>(rows + k * stride, stride, 0, lens ? lens[k] : stride, maxFrames, ackSlots, ackBytes,
                           scratchRecs + k * maxFrames * 32, scratchSlots + k * ackSlots * ackBytes, &acks, nullptr);
    *reinterpret_cast<GMEM uint32_t*>(scratchCounts + k * 4) = acks < ackSlots ? acks : ackSlots;
}

// k_ackstreamwalk (ops.h duplex_streams_bytes): k_ackwalkd for rows that are
// byte streams -- the same lane per row and the same scratch areas, the walk in
// its stream mode over row bytes [starts[k], ends[k]), and the row's next word
// behind the output's dense part.  The row word may carry kStreamPartialDuplex;
// k_rowsum2 masks the word with kPackedCountMask before it sums, so the flag
// rides along as the others do, and k_compact and k_slots read only the tables:
// all three run unchanged behind this walk.  No LDS, no atomics.
__global__ __launch_bounds__(kAckStreamWalkThreads) void k_ackstreamwalk(
    uint64_t rows, uint64_t stride, const uint32_t* __restrict__ starts, const uint32_t* __restrict__ ends,
    uint32_t count, uint32_t maxFrames, uint32_t ackSlots, uint32_t ackBytes, uint64_t scratchRecs,
    uint64_t scratchSlots, uint64_t scratchCounts, uint64_t words, uint64_t nexts)
{
    const uint64_t k = (uint64_t)blockIdx.x * kAckStreamWalkThreads + threadIdx.x;
    if (k >= count)
        return;
    uint32_t acks = 0;
    uint64_t next = 0;
    *reinterpret_cast<GMEM uint32_t*>(words + k * 4) = ackwalk_row<true>(
        rows + k * stride, stride, starts ? starts[k] : 0, ends ? ends[k] : stride, maxFrames, ackSlots, ackBytes,
        scratchRecs + k * maxFrames * 32, scratchSlots + k * ackSlots * ackBytes, &acks, &next);
    *reinterpret_cast<GMEM uint32_t*>(scratchCounts + k * 4) = acks < ackSlots ? acks : ackSlots;
    *reinterpret_cast<GMEM uint32_t*>(nexts + k * 4) = next < 0xffffffffull ? (uint32_t)next : 0xffffffffu;
    // the zeros between the next words and the next 16-byte boundary: every byte is written by every scan
    if (k + 1 == count)
        for (uint64_t j = count; j < (((uint64_t)count + 3) & ~(uint64_t)3); ++j)
            *reinterpret_cast<GMEM uint32_t*>(nexts + j * 4) = 0;
}

// wave_incl_sum on two 32-bit sums at once, the records' in the low half and
// the acks' in the high half: neither can carry into the other, both totals
// being below 2^32 (in fact below 2^27: the duplex scan's own size limit)
__device__ __forceinline__ uint64_t wave_incl_sum2(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (unsigned s = 1; s < 64; s <<= 1) {
        const uint64_t u = __shfl_up(v, s);
        if (lane >= s)
            v += u;
    }
    return v;
}

// k_rowsum2: k_rowsum's carry scheme -- one workgroup striding over the rows,
// kRowsum2Rows consecutive rows per lane, per pass the lane sums, a wave scan,
// the wave sums through a double-buffered LDS table behind one barrier, the
// carry of the passes before in a register -- over the record counts (the row
// words, clamped to maxFrames) and the ack counts (the scratch count table,
// clamped to ackSlots) in one pass, so a row's scratch spans can never be left
// whatever the tables hold.  It writes start[], astart[], the padding behind
// each and the info words {T, W, c, WA}.  A row is complete while start[k + 1]
// <= maxRecords and astart[k + 1] <= maxAcks; both sequences only grow, so the
// number of such rows is c and the largest such starts are W and WA: c is joint
// over the two tables, which is why this is one kernel and not k_rowsum run
// twice.  Integers, a fixed order, no atomics.
__global__ __launch_bounds__(kRowsum2Threads) void k_rowsum2(uint64_t out, uint64_t counts, uint32_t count,
                                                             uint32_t maxFrames, uint32_t ackSlots,
                                                             uint32_t maxRecords, uint32_t maxAcks)
{
    constexpr uint32_t kWaves = kRowsum2Threads / 64;
    __shared__ uint64_t wsum[2][kWaves];
    __shared__ uint32_t redC[kWaves], redW[kWaves], redA[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t words = out + 16, starts = words + (uint64_t)count * 4;
    const uint64_t astarts = out + duplex_dense_acks_offset(count, maxRecords);
    auto load = [&](uint32_t base, uint64_t* n) {
        const uint64_t r0 = (uint64_t)base + tid * kRowsum2Rows;
        uint32_t f[kRowsum2Rows], a[kRowsum2Rows];
        if (r0 + kRowsum2Rows <= count) {   // (16-byte aligned: base and kRowsum2Rows are multiples of 4)
            const uint4 x = ld16(words + r0 * 4), y = ld16(words + r0 * 4 + 16);
            const uint4 p = ld16(counts + r0 * 4), q = ld16(counts + r0 * 4 + 16);
            f[0] = x.x, f[1] = x.y, f[2] = x.z, f[3] = x.w;
            f[4] = y.x, f[5] = y.y, f[6] = y.z, f[7] = y.w;
            a[0] = p.x, a[1] = p.y, a[2] = p.z, a[3] = p.w;
            a[4] = q.x, a[5] = q.y, a[6] = q.z, a[7] = q.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kRowsum2Rows; ++j) {
                const bool in = r0 + j < count;
                f[j] = in ? *reinterpret_cast<const GMEM uint32_t*>(words + (r0 + j) * 4) : 0u;
                a[j] = in ? *reinterpret_cast<const GMEM uint32_t*>(counts + (r0 + j) * 4) : 0u;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kRowsum2Rows; ++j) {
            f[j] &= kPackedCountMask;
            f[j] = f[j] < maxFrames ? f[j] : maxFrames;
            a[j] = a[j] < ackSlots ? a[j] : ackSlots;
            n[j] = (uint64_t)f[j] | ((uint64_t)a[j] << 32);
        }
    };
    static_assert(kRowsum2Rows == 8, "k_rowsum2 loads a lane's rows as two 16-byte words per table");
    uint64_t carry = 0;
    uint32_t done = 0, W = 0, WA = 0;
    uint64_t nx[kRowsum2Rows];
    load(0, nx);
    for (uint32_t base = 0, p = 0; base < count; base += kRowsum2Pass, p ^= 1) {
        uint64_t n[kRowsum2Rows];
        uint64_t s = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRowsum2Rows; ++j) {
            n[j] = nx[j];
            s += n[j];
        }
        if (count - base > kRowsum2Pass)
            load(base + kRowsum2Pass, nx);
        const uint64_t incl = wave_incl_sum2(s, lane);
        if (lane == 63)
            wsum[p][wave] = incl;
        __syncthreads();
        uint64_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint64_t v = wsum[p][w];
            total += v;
            before += w < wave ? v : 0ull;
        }
        uint64_t at = carry + before + incl - s;
        const uint64_t r0 = (uint64_t)base + tid * kRowsum2Rows;
#pragma unroll
        for (uint32_t j = 0; j < kRowsum2Rows; ++j) {
            if (r0 + j < count) {
                *reinterpret_cast<GMEM uint32_t*>(starts + (r0 + j) * 4) = (uint32_t)at;
                *reinterpret_cast<GMEM uint32_t*>(astarts + (r0 + j) * 4) = (uint32_t)(at >> 32);
                at += n[j];
                if ((uint32_t)at <= maxRecords && (uint32_t)(at >> 32) <= maxAcks) {
                    ++done;
                    W = (uint32_t)at;
                    WA = (uint32_t)(at >> 32);
                }
            }
        }
        carry += total;
    }
    // c = the sum of done, W and WA = the largest ones (0 where no row is complete)
#pragma unroll
    for (unsigned s = 32; s >= 1; s >>= 1) {
        done += __shfl_xor(done, s);
        const uint32_t o = __shfl_xor(W, s), oa = __shfl_xor(WA, s);
        W = W > o ? W : o;
        WA = WA > oa ? WA : oa;
    }
    if (lane == 0) {
        redC[wave] = done;
        redW[wave] = W;
        redA[wave] = WA;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0, w = 0, wa = 0;
        for (uint32_t i = 0; i < kWaves; ++i) {
            c += redC[i];
            w = w > redW[i] ? w : redW[i];
            wa = wa > redA[i] ? wa : redA[i];
        }
        *reinterpret_cast<GMEM uint32_t*>(starts + (uint64_t)count * 4) = (uint32_t)carry;
        for (uint64_t a = starts + (uint64_t)(count + 1) * 4; a < out + dense_records_offset(count); a += 4)
            *reinterpret_cast<GMEM uint32_t*>(a) = 0;
        *reinterpret_cast<GMEM uint32_t*>(astarts + (uint64_t)count * 4) = (uint32_t)(carry >> 32);
        for (uint64_t a = astarts + (uint64_t)(count + 1) * 4; a < out + duplex_dense_slots_offset(count, maxRecords);
             a += 4)
            *reinterpret_cast<GMEM uint32_t*>(a) = 0;
        st16(out, make_uint4((uint32_t)carry, w, c, wa));
    }
}

// k_slots: one 16-byte word of the output's slot area per lane, over all
// maxAcks * ackBytes / 16 words: a wave stores 1 KiB of consecutive bytes.
// Slot i < WA belongs to the row k with astart[k] <= i < astart[k + 1] (rows
// without a slot share a start with the next row and own none): a binary search
// over astart[0, c], whose two ends hold 0 and WA, so k < c always; the table
// stays in cache.  The word comes from slot i - astart[k] of row k's scratch
// slots (below ackSlots, by k_rowsum2's clamp); a word from WA on is zero.  No
// LDS, no atomics.
__global__ __launch_bounds__(kSlotsThreads) void k_slots(uint64_t out, uint64_t scratchSlots, uint32_t count,
                                                         uint32_t ackSlots, uint32_t ackBytes, uint32_t maxRecords,
                                                         uint32_t maxAcks)
{
    const uint64_t g = (uint64_t)blockIdx.x * kSlotsThreads + threadIdx.x;
    const uint32_t per = ackBytes >> 4;   // 16-byte words per slot
    if (g >= (uint64_t)maxAcks * per)
        return;
    const uint64_t i = g / per, o = (g - i * per) * 16;
    const uint4 info = ld16(out);   // {T, W, c, WA}
    const uint32_t c = info.z < count ? info.z : count;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i < info.w && c != 0) {
        const uint64_t astarts = out + duplex_dense_acks_offset(count, maxRecords);
        uint32_t lo = 0, hi = c;   // astart[lo] <= i < astart[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (*reinterpret_cast<const GMEM uint32_t*>(astarts + (uint64_t)mid * 4) <= i)
                lo = mid;
            else
                hi = mid;
        }
        const uint64_t j = i - *reinterpret_cast<const GMEM uint32_t*>(astarts + (uint64_t)lo * 4);
        if (j < ackSlots)
            v = ld16(scratchSlots + ((uint64_t)lo * ackSlots + j) * ackBytes + o);
    }
    st16(out + duplex_dense_slots_offset(count, maxRecords) + g * 16, v);
}

// ---------------------------------------------------------------------------
// Host side

namespace {

hipStream_t g_stream = nullptr;
hipStream_t g_stageStream = nullptr;    // application H2D staging (be_stage_h2d)
hipStream_t g_gatherStream = nullptr;   // gathers of completed results (be_gather)
// the side stream of a submission with device recovery-matrix jobs: the rest
// of the upload and k_ingest beside k_ge, or k_ge beside the codec stream
// (be_launch_ge / be_side_upload_ingest / be_join_ge)
hipStream_t g_geStream = nullptr;
hipEvent_t g_geFork = nullptr, g_geJoin = nullptr;
bool g_gePending = false;   // (launcher thread only)
bool g_ready = false;
int g_device = 0;

// The HIP current device is per host thread, and codec calls (buffer
// allocation) run on the application's threads: make each thread that
// reaches the backend use the engine's device (one process per GPU, the
// device chosen at init).
inline void bind_device()
{
    thread_local int bound = -1;
    if (bound != g_device) {
        (void)hipSetDevice(g_device);
        bound = g_device;
    }
}
bool g_timing = false;
// window elements an OP_ROWS batch stages in LDS per tile (256 B each, beside
// the 24 sums); sized at init to the LDS the kernel's static arrays leave
// free; SGPU_STAGE overrides (0 = read every element from memory)
uint32_t g_stageCap = 0;
double g_totalMs = 0;
double g_kernelMs[kBeKernelKinds] = {};   // by BeKernel

struct EvPair
{
    hipEvent_t a, b;
    BeKernel kind;
};
// Launches come from the engine's launcher thread, fence waits from its
// completer thread: the event lists are shared under g_evMu.
std::mutex g_evMu;
std::vector<EvPair> g_evFree;
std::deque<EvPair> g_evUsed;
std::vector<hipEvent_t> g_fenceFree;

EvPair take_events(BeKernel kind)
{
    EvPair e;
    {
        std::lock_guard<std::mutex> g(g_evMu);
        if (!g_evFree.empty()) {
            e = g_evFree.back();
            g_evFree.pop_back();
            e.kind = kind;
            return e;
        }
    }
    (void)hipEventCreate(&e.a);
    (void)hipEventCreate(&e.b);
    e.kind = kind;
    return e;
}

struct Timed
{
    EvPair ev;
    bool on;
    hipStream_t stream;
    explicit Timed(BeKernel kind, hipStream_t s = nullptr) : on(g_timing), stream(s ? s : g_stream)
    {
        bind_device();
        if (on) {
            ev = take_events(kind);
            (void)hipEventRecord(ev.a, stream);
        }
    }
    ~Timed()
    {
        if (on) {
            (void)hipEventRecord(ev.b, stream);
            std::lock_guard<std::mutex> g(g_evMu);
            g_evUsed.push_back(ev);
        }
    }
};

// Fold the timing events that have completed (in stream order) into the
// totals.  all = true after a full stream synchronisation.
void harvest_timing(bool all)
{
    std::lock_guard<std::mutex> g(g_evMu);
    while (!g_evUsed.empty()) {
        const EvPair& ev = g_evUsed.front();
        if (!all && hipEventQuery(ev.b) != hipSuccess)
            break;
        // (a synchronised codec stream says nothing about the gather stream)
        if (all && (ev.kind == kBeScan || ev.kind == kBeWalk || ev.kind == kBeAckWalk || ev.kind == kBeRowsum ||
                    ev.kind == kBeCompact || ev.kind == kBeRowsum2 || ev.kind == kBeSlots ||
                    ev.kind == kBeStreamWalk || ev.kind == kBeAckStreamWalk))
            (void)hipEventSynchronize(ev.b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev.a, ev.b);
        g_totalMs += ms;
        g_kernelMs[ev.kind] += ms;
        g_evFree.push_back(ev);
        g_evUsed.pop_front();
    }
}

void check(hipError_t e, const char* what)
{
    if (e != hipSuccess) {
        std::fprintf(stderr, "siamese_amd: %s failed: %s\n", what, hipGetErrorString(e));
    }
}

} // namespace

bool be_init(int device, const char** err)
{
    if (g_ready)
        return true;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        *err = "no HIP device visible: libsiamese_amd requires an MI355X (gfx950)";
        return false;
    }
    if (device >= 0 && hipSetDevice(device) != hipSuccess) {
        *err = "hipSetDevice failed";
        return false;
    }
    int cur = 0;
    (void)hipGetDevice(&cur);
    g_device = cur;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cur) != hipSuccess) {
        *err = "hipGetDeviceProperties failed";
        return false;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        *err = "device is not gfx950 (MI355X); kernels are built for gfx950 only";
        return false;
    }
    // Host threads next to the device: the NUMA node of its PCI function,
    // a slice per device on that node (placement.h).
    {
        char bus[64] = {0};
        auto node_of = [](const char* b) {
            std::string s(b);
            for (char& c : s)
                c = (char)std::tolower((unsigned char)c);
            FILE* f = std::fopen(("/sys/bus/pci/devices/" + s + "/numa_node").c_str(), "r");
            int node = -1;
            if (f) {
                if (std::fscanf(f, "%d", &node) != 1)
                    node = -1;
                std::fclose(f);
            }
            return node;
        };
        if (hipDeviceGetPCIBusId(bus, sizeof(bus), cur) == hipSuccess) {
            const int myNode = node_of(bus);
            unsigned slice = 0;
            for (int d = 0; d < cur; ++d) {
                char other[64] = {0};
                if (hipDeviceGetPCIBusId(other, sizeof(other), d) == hipSuccess &&
                    node_of(other) == myNode)
                    ++slice;
            }
            place_near_device(bus, slice, WorkerPool::default_threads());
        }
    }
    if (hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking) != hipSuccess) {
        *err = "hipStreamCreate failed";
        return false;
    }
    if (hipStreamCreateWithFlags(&g_stageStream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&g_gatherStream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&g_geStream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&g_geFork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g_geJoin, hipEventDisableTiming) != hipSuccess) {
        *err = "hipStreamCreate (transfer streams) failed";
        return false;
    }
    if (!gf_init()) {
        *err = "GF(256) table self-check failed";
        return false;
    }
    static uint32_t perm[256][8];
    for (unsigned y = 0; y < 256; ++y) {
        uint8_t ta[8], tb[8], tc[4];
        for (unsigned k = 0; k < 8; ++k) {
            ta[k] = gf_mul((uint8_t)k, (uint8_t)y);
            tb[k] = gf_mul((uint8_t)(k << 3), (uint8_t)y);
        }
        for (unsigned k = 0; k < 4; ++k)
            tc[k] = gf_mul((uint8_t)(k << 6), (uint8_t)y);
        std::memset(perm[y], 0, sizeof(perm[y]));
        std::memcpy(&perm[y][0], ta, 8);
        std::memcpy(&perm[y][2], tb, 8);
        std::memcpy(&perm[y][4], tc, 4);
    }
    check(hipMemcpyToSymbol(HIP_SYMBOL(c_perm), perm, sizeof(perm)), "hipMemcpyToSymbol(perm)");
    check(hipMemcpyToSymbol(HIP_SYMBOL(c_inv), g_gf.inv, 256), "hipMemcpyToSymbol(inv)");
    check(hipMemcpyToSymbol(HIP_SYMBOL(c_sqr), g_gf.sqr, 256), "hipMemcpyToSymbol(sqr)");
    // PCG jump-ahead: state after j draws = A^j s + inc * (A^0 + ... + A^(j-1))
    uint64_t pa[65], pg[65];
    pa[0] = 1;
    pg[0] = 0;
    for (unsigned j = 1; j <= 64; ++j) {
        pa[j] = pa[j - 1] * kPcgMul;
        pg[j] = pg[j - 1] * kPcgMul + 1;
    }
    check(hipMemcpyToSymbol(HIP_SYMBOL(c_pcgA), pa, sizeof(pa)), "hipMemcpyToSymbol(pcgA)");
    // jumps of 2^k draws: A^(2^k) and sum_{t<2^k} A^t
    uint64_t ja[32], jg[32];
    ja[0] = kPcgMul;
    jg[0] = 1;
    for (unsigned k = 1; k < 32; ++k) {
        jg[k] = jg[k - 1] * ja[k - 1] + jg[k - 1];
        ja[k] = ja[k - 1] * ja[k - 1];
    }
    check(hipMemcpyToSymbol(HIP_SYMBOL(c_pcgJA), ja, sizeof(ja)), "hipMemcpyToSymbol(pcgJA)");
    check(hipMemcpyToSymbol(HIP_SYMBOL(c_pcgJG), jg, sizeof(jg)), "hipMemcpyToSymbol(pcgJG)");
    {
        hipFuncAttributes fa;
        size_t staticLds = 64u * 1024u;
        if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_exec)) == hipSuccess)
            staticLds = fa.sharedSizeBytes;
        const size_t ldsPerCu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor
                                                                : 160u * 1024u;
        const size_t dyn = ldsPerCu > staticLds ? ldsPerCu - staticLds : 0;
        // (the sums, the window and one zero slot)
        g_stageCap = dyn / kExecTileBytes > kRowSums + 1 ? (uint32_t)(dyn / kExecTileBytes) - kRowSums - 1 : 0;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_exec),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((kRowSums + g_stageCap + 1) * kExecTileBytes)) != hipSuccess)
            g_stageCap = 48u * 1024u / kExecTileBytes - kRowSums - 1;
    }
    check(hipMemcpyToSymbol(HIP_SYMBOL(c_pcgG), pg, sizeof(pg)), "hipMemcpyToSymbol(pcgG)");
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_solve_main),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)solve_launch_lds_bytes(kSolveLdsMaxRows)) != hipSuccess) {
        *err = "the device refused the triangular solve's LDS (gfx950 grants 160 KiB per workgroup)";
        return false;
    }
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_solve_tr), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)solve_tr_lds_bytes(kProductMaxRows)) != hipSuccess) {
        *err = "the device refused the vector product solve's LDS";
        return false;
    }
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_solve_pre), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)solve_pre_lds_bytes(kSolveLdsMaxRows)) != hipSuccess) {
        *err = "the device refused the solve pre-pass's LDS";
        return false;
    }
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_solve_prefix),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)solve_prefix_lds_bytes(kSolveLdsMaxRows)) != hipSuccess) {
        *err = "the device refused the solve prefix pass's LDS";
        return false;
    }
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ge), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)ge_lds_bytes(kGeMaxRows, kGeMaxCols)) != hipSuccess) {
        *err = "the device refused the recovery matrix's LDS";
        return false;
    }
    if (hipDeviceSynchronize() != hipSuccess) {
        *err = "device synchronisation failed during init";
        return false;
    }
    g_ready = true;
    return true;
}

const char* be_name() { return "hip-gfx950"; }

uint32_t be_exec_stage_cap() { return g_stageCap; }


#ifdef SGPU_PHASE_CLOCKS
extern "C" __attribute__((visibility("default"))) void sgpu_debug_phase_clocks(unsigned long long* out32)
{
    bind_device();
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_phaseClk), 64 * sizeof(unsigned long long));
}
#endif

void* be_dev_alloc(size_t bytes)
{
    bind_device();
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess)
        return nullptr;
    return p;
}

void be_dev_free(void* p)
{
    bind_device();
    if (p)
        (void)hipFree(p);
}

void* be_host_alloc(size_t bytes)
{
    bind_device();
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess)
        return nullptr;
    return p;
}

void* be_host_alloc_mapped(size_t bytes)
{
    bind_device();
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return nullptr;
    return p;
}

void* be_host_device_ptr(void* host)
{
    bind_device();
    void* d = nullptr;
    return hipHostGetDevicePointer(&d, host, 0) == hipSuccess ? d : nullptr;
}

void be_host_free(void* p)
{
    bind_device();
    if (p)
        (void)hipHostFree(p);
}

void be_h2d(void* dst, const void* src, size_t bytes)
{
    bind_device();
    check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g_stream), "H2D");
}

void be_d2h(void* dst, const void* src, size_t bytes)
{
    bind_device();
    check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g_stream), "D2H");
}

namespace {
constexpr uint64_t kKernelCopyMax = 256u << 10;   // total bytes a be_copy_pinned kernel moves at most
constexpr unsigned kHostCopyThreads = 256;
struct HostCopyArgs
{
    BeCopy r[kBeCopyMax];
    uint32_t count;
};
} // namespace

// Pinned host <-> device copies as a kernel (be_copy_pinned): blockIdx.y is
// the range, each thread moves 16-byte words (bytes at the unaligned ends);
// host memory is page-locked and mapped, written with ordinary stores.
__device__ __forceinline__ void copy_range(const BeCopy& c)
{
    uint8_t* dst = reinterpret_cast<uint8_t*>(c.dst);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(c.src);
    const uint64_t n = c.bytes;
    const bool aligned = ((c.dst | c.src) & 15u) == 0;
    const uint64_t words = aligned ? n / 16 : 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kHostCopyThreads + threadIdx.x; i < words;
         i += (uint64_t)gridDim.x * kHostCopyThreads)
        reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    for (uint64_t i = words * 16 + (uint64_t)blockIdx.x * kHostCopyThreads + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * kHostCopyThreads)
        dst[i] = src[i];
}

__global__ __launch_bounds__(kHostCopyThreads) void k_hostcopy(HostCopyArgs a) { copy_range(a.r[blockIdx.y]); }

// The same from a device-readable range list (be_copy_list).
__global__ __launch_bounds__(kHostCopyThreads) void k_copylist(const BeCopy* __restrict__ list)
{
    copy_range(list[blockIdx.y]);
}

void be_copy_pinned(const BeCopy* ranges, unsigned count, bool toDevice)
{
    bind_device();
    uint64_t total = 0, most = 0;
    for (unsigned i = 0; i < count; ++i) {
        total += ranges[i].bytes;
        most = std::max<uint64_t>(most, ranges[i].bytes);
    }
    if (count == 0 || total == 0)
        return;
    if (count > kBeCopyMax || total > kKernelCopyMax) {
        for (unsigned i = 0; i < count; ++i)
            if (ranges[i].bytes)
                check(hipMemcpyAsync((void*)(uintptr_t)ranges[i].dst, (const void*)(uintptr_t)ranges[i].src,
                                     ranges[i].bytes, toDevice ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost,
                                     g_stream),
                      toDevice ? "H2D" : "D2H");
        return;
    }
    HostCopyArgs a;
    std::memset(&a, 0, sizeof(a));
    for (unsigned i = 0; i < count; ++i) {
        a.r[i] = ranges[i];
        // the host side as the device addresses it (mapped pinned memory)
        uint64_t& h = toDevice ? a.r[i].src : a.r[i].dst;
        void* d = nullptr;
        if (hipHostGetDevicePointer(&d, (void*)(uintptr_t)h, 0) == hipSuccess && d)
            h = (uint64_t)(uintptr_t)d;
    }
    a.count = count;
    const uint64_t perBlock = (uint64_t)kHostCopyThreads * 16u * 4u;   // four words per thread
    const unsigned blocks = (unsigned)std::min<uint64_t>(64, (most + perBlock - 1) / perBlock);
    hipLaunchKernelGGL(k_hostcopy, dim3(std::max(1u, blocks), count), dim3(kHostCopyThreads), 0, g_stream, a);
}

void be_copy_list(const BeCopy* ranges, const void* devList, unsigned count, bool toDevice)
{
    uint64_t total = 0, most = 0;
    for (unsigned i = 0; i < count; ++i) {
        total += ranges[i].bytes;
        most = std::max<uint64_t>(most, ranges[i].bytes);
    }
    if (count <= kBeCopyMax || !devList || total > kKernelCopyMax || count > 65535u) {
        be_copy_pinned(ranges, count, toDevice);
        return;
    }
    bind_device();
    const uint64_t perBlock = (uint64_t)kHostCopyThreads * 16u * 4u;   // four words per thread
    const unsigned blocks = (unsigned)std::min<uint64_t>(64, (most + perBlock - 1) / perBlock);
    hipLaunchKernelGGL(k_copylist, dim3(std::max(1u, blocks), count), dim3(kHostCopyThreads), 0, g_stream,
                       static_cast<const BeCopy*>(devList));
}

void be_memset(void* dst, int value, size_t bytes)
{
    bind_device();
    check(hipMemsetAsync(dst, value, bytes, g_stream), "memset");
}

namespace {

// k_ingest on `stream` (the codec stream, or the side stream beside the
// matrix jobs)
void launch_ingest(const BeIngest& in, hipStream_t stream)
{
    const uint32_t chunks = in.maxBytes ? (in.maxBytes + kIngestChunkBytes - 1) / kIngestChunkBytes : 1;
    const uint32_t grid = in.blocks ? in.nblocks : (in.count + kIngestWaves - 1) / kIngestWaves;
    if (in.count == 0 || grid == 0)
        return;
    Timed t(kBeIngest, stream);
    hipLaunchKernelGGL(k_ingest, dim3(grid, chunks), dim3(64 * kIngestWaves), 0, stream, in.descs, in.count,
                       in.blocks);
}

} // namespace

void be_launch_ingest(const BeIngest& ingest)
{
    launch_ingest(ingest, g_stream);
}

void be_launch_deliver(const DeliverItem* items, uint32_t count, uint32_t maxStride)
{
    if (count == 0)
        return;
    Timed t(kBeDeliver);
    // (a wave walks the chunks of a row the grid is too short for)
    const uint32_t chunks =
        std::min(kDeliverMaxChunks, std::max(1u, (uint32_t)(((uint64_t)maxStride + kIngestChunkBytes - 1) / kIngestChunkBytes)));
    hipLaunchKernelGGL(k_deliver, dim3((count + kDeliverWaves - 1) / kDeliverWaves, chunks), dim3(64 * kDeliverWaves), 0,
                       g_stream, items, count);
}

void be_launch_frame(const FrameItem* items, uint32_t count, uint32_t maxStride)
{
    if (count == 0)
        return;
    Timed t(kBeFrame);
    // (the grid of be_launch_deliver)
    const uint32_t chunks =
        std::min(kDeliverMaxChunks, std::max(1u, (uint32_t)(((uint64_t)maxStride + kIngestChunkBytes - 1) / kIngestChunkBytes)));
    hipLaunchKernelGGL(k_frame, dim3((count + kDeliverWaves - 1) / kDeliverWaves, chunks), dim3(64 * kDeliverWaves), 0,
                       g_stream, items, count);
}

void be_launch_relay(const RelayItem* items, uint32_t count, uint32_t maxStride)
{
    if (count == 0)
        return;
    Timed t(kBeRelay);
    // (the grid of be_launch_deliver)
    const uint32_t chunks =
        std::min(kDeliverMaxChunks, std::max(1u, (uint32_t)(((uint64_t)maxStride + kIngestChunkBytes - 1) / kIngestChunkBytes)));
    hipLaunchKernelGGL(k_relay, dim3((count + kDeliverWaves - 1) / kDeliverWaves, chunks), dim3(64 * kDeliverWaves), 0,
                       g_stream, items, count);
}

void be_launch_pack(const PackJob* jobs, uint32_t jobCount, const PackItem* items, uint32_t count, PlanRec* plan,
                    uint32_t maxStride)
{
    if (jobCount == 0)
        return;
    {
        Timed t(kBePlan);
        hipLaunchKernelGGL(k_plan, dim3((jobCount + kDeliverWaves - 1) / kDeliverWaves), dim3(64 * kDeliverWaves), 0,
                           g_stream, jobs, jobCount, items, plan);
    }
    if (count == 0)   // (jobs without items: their length words and info records were all there is)
        return;
    Timed t(kBePack);
    // (the grid of be_launch_deliver: a span is at most a row)
    const uint32_t chunks =
        std::min(kDeliverMaxChunks, std::max(1u, (uint32_t)(((uint64_t)maxStride + kIngestChunkBytes - 1) / kIngestChunkBytes)));
    hipLaunchKernelGGL(k_pack, dim3((count + kDeliverWaves - 1) / kDeliverWaves, chunks), dim3(64 * kDeliverWaves), 0,
                       g_stream, jobs, items, (const PlanRec*)plan, count);
}

void be_launch_concat(const ConcatJob* jobs, uint32_t jobCount, const ConcatItem* items, uint32_t count,
                      ConcatRec* recs, uint32_t maxBytes)
{
    if (jobCount == 0)
        return;
    {
        Timed t(kBeOffsets);
        hipLaunchKernelGGL(k_offsets, dim3((jobCount + kDeliverWaves - 1) / kDeliverWaves), dim3(64 * kDeliverWaves),
                           0, g_stream, jobs, jobCount, items, recs);
    }
    if (count == 0)   // (jobs without items: their offset words and info records were all there is)
        return;
    Timed t(kBeConcat);
    // (the grid of be_launch_deliver: a payload is shorter than its symbol, and starts up to 15 bytes into a word)
    const uint32_t chunks = std::min(
        kDeliverMaxChunks, std::max(1u, (uint32_t)(((uint64_t)maxBytes + 15 + kIngestChunkBytes - 1) / kIngestChunkBytes)));
    hipLaunchKernelGGL(k_concat, dim3((count + kDeliverWaves - 1) / kDeliverWaves, chunks), dim3(64 * kDeliverWaves), 0,
                       g_stream, jobs, items, (const ConcatRec*)recs, count);
}

void be_launch_exec(const void* stream, const ExecItem* items, uint32_t count, uint64_t* acct,
                    const uint32_t* results, uint32_t maxWindow)
{
    if (count == 0)
        return;
    Timed t(kBeExec);
    // LDS stage: the 24 sums plus the largest OP_ROWS window of the launch,
    // up to the device's budget (none for launches without row batches)
    uint32_t slots = 0;
    if (maxWindow != kNoRows)
        slots = kRowSums + (maxWindow < g_stageCap ? maxWindow : g_stageCap);
    hipLaunchKernelGGL(k_exec, dim3(count), dim3(kExecThreads), (size_t)(slots ? slots + 1 : 0) * kExecTileBytes,
                       g_stream, static_cast<const uint4*>(stream), items,
                       reinterpret_cast<unsigned long long*>(acct), results, slots);
}

void be_launch_ldpc(const LdpcItem* items, uint32_t count, uint64_t* acct, const uint32_t* gates,
                    const uint32_t* results)
{
    if (count == 0)
        return;
    Timed t(kBeLdpc);
    if (!gates)
        hipLaunchKernelGGL(k_ldpc<false>, dim3(count), dim3(64 * kLdpcWaves), 0, g_stream, items,
                           reinterpret_cast<unsigned long long*>(acct), (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr);
    else
        hipLaunchKernelGGL(k_ldpc<true>, dim3(count), dim3(64 * kLdpcWaves), 0, g_stream, items,
                           reinterpret_cast<unsigned long long*>(acct), gates, results);
}

void be_launch_ge(const BeGe& ge, GePlace place, const BeCopy& head)
{
    if (ge.count == 0)
        return;
    // The side stream starts after everything the codec stream queued before
    // this submission's matrix jobs (an application may pass the output of an
    // earlier submission as an original: k_ingest must not read it early).
    check(hipEventRecord(g_geFork, g_stream), "hipEventRecord(ge fork)");
    check(hipStreamWaitEvent(g_geStream, g_geFork, 0), "hipStreamWaitEvent(ge fork)");
    // kCodecStream: the jobs in line, be_side_upload_ingest puts the rest of
    // the upload and k_ingest beside them after the fork (a cross-stream wait
    // costs 16-23 us before the next kernel even when satisfied, and the join
    // behind jobs on the side stream waited on a job that ended about when
    // k_ingest did: profiles/r6l_ge_codec_stream_ab.txt).  kSideStream: the
    // jobs beside the codec stream's next launches until be_join_ge.
    const bool side = place == GePlace::kSideStream;
    hipStream_t stream = side ? g_geStream : g_stream;
    if (!side && head.bytes)
        check(hipMemcpyAsync((void*)(uintptr_t)head.dst, (const void*)(uintptr_t)head.src, head.bytes,
                             hipMemcpyHostToDevice, g_stream),
              "H2D (ge head)");
    {
        Timed t(kBeGe, stream);
        hipLaunchKernelGGL(k_ge, dim3(ge.count), dim3(kGeThreads), (size_t)ge_lds_bytes(ge.maxRows, ge.maxCols),
                           stream, ge.descs, ge.in, ge.results, ge.rows, ge.coef, ge.rowsIn);
    }
    if (side) {
        check(hipEventRecord(g_geJoin, g_geStream), "hipEventRecord(ge join)");
        g_gePending = true;
    }
}

void be_side_upload_ingest(const BeCopy& rest, const BeIngest& ingest)
{
    bind_device();
    if (rest.bytes)
        check(hipMemcpyAsync((void*)(uintptr_t)rest.dst, (const void*)(uintptr_t)rest.src, rest.bytes,
                             hipMemcpyHostToDevice, g_geStream),
              "H2D (upload rest)");
    launch_ingest(ingest, g_geStream);
    check(hipEventRecord(g_geJoin, g_geStream), "hipEventRecord(side join)");
    g_gePending = true;
}

void be_join_ge()
{
    if (!g_gePending)
        return;
    check(hipStreamWaitEvent(g_stream, g_geJoin, 0), "hipStreamWaitEvent(ge join)");
    g_gePending = false;
}

namespace {

// How a split launch runs (solve_split; the others always take the fused
// sweeps)
enum SolvePath
{
    kPathSweeps = 0,   // k_solve_prefix + k_solve_main
    kPathVector = 2,   // k_solve_pre + k_solve_tr + k_solve_main
};

void launch_solve(const SolveDesc* solves, const SolveRow* rows, const uint8_t* coef, uint32_t* results,
                  const SolveItem* items, uint32_t count, uint32_t maxRows, uint64_t* acct, uint32_t solveBegin,
                  uint32_t solveCount, SolvePath path)
{
    const uint32_t rowsCap = maxRows < kSolveLdsMaxRows ? maxRows : kSolveLdsMaxRows;
    // Many solves or large ones: their prefixes in one wave each first (once
    // per solve, all in parallel); few small ones (single-stream flushes):
    // fused into the tiles, one launch fewer on the flush's critical path.
    const bool separate = solve_split(solveCount, maxRows);
    const bool tr = separate && path == kPathVector;
    unsigned long long* acctL = reinterpret_cast<unsigned long long*>(acct);
    const uint32_t prodCap = rowsCap < kProductMaxRows ? rowsCap : kProductMaxRows;
    if (tr) {
        hipLaunchKernelGGL(k_solve_pre, dim3(2 * solveCount), dim3(kPreThreads), (size_t)solve_pre_lds_bytes(rowsCap),
                           g_stream, solves + solveBegin, rows, coef, results, acctL, solveCount, 0u);
        hipLaunchKernelGGL(k_solve_tr, dim3(count * kTrSplit * kTrHalves), dim3(kTrThreads), (size_t)solve_tr_lds_bytes(prodCap),
                           g_stream, solves, rows, results, items);
    } else if (separate) {
        hipLaunchKernelGGL(k_solve_prefix, dim3(solveCount), dim3(64), (size_t)solve_prefix_lds_bytes(rowsCap),
                           g_stream, solves + solveBegin, rows, coef, results, acctL);
    }
    hipLaunchKernelGGL(k_solve_main, dim3(count), dim3(64 * kSolveWaves),
                       (size_t)solve_launch_lds_bytes(rowsCap, !separate), g_stream, solves, rows, coef, results,
                       items, acctL, (separate ? 1u : 0u) | (tr ? 4u : 0u));
}

} // namespace

namespace {

// Default: the solves whose lengths all come out valid as X = T R on the
// vector ALUs (k_solve_pre 80 + k_solve_tr 103 + k_solve_main 9 us per
// headline launch against k_solve_prefix 58 + k_solve_main 277 for the
// sweeps; profiles/r4ac_*).  SGPU_TR_SOLVE=0: the sweeps alone (a test knob:
// test_product_solve_paths runs the hashed fixtures through them).
SolvePath solve_path()
{
    static const SolvePath kPath = [] {
        const char* v = std::getenv("SGPU_TR_SOLVE");
        return (!v || std::atoi(v) != 0) ? kPathVector : kPathSweeps;
    }();
    return kPath;
}

} // namespace

void be_launch_solve(const SolveDesc* solves, const SolveRow* rows, const uint8_t* coef, uint32_t* results,
                     const SolveItem* items, uint32_t count, uint32_t maxRows, uint64_t* acct,
                     uint32_t solveBegin, uint32_t solveCount)
{
    if (count == 0)
        return;
    Timed t(kBeSolve);
    launch_solve(solves, rows, coef, results, items, count, maxRows, acct, solveBegin, solveCount, solve_path());
}

// Test hook: the solve paths against one another on random systems.  Builds
// `nsolves` solves of 16..120 rows (split launches: solve_split) whose true rows carry
// valid length prefixes and zero bytes past their lengths, as the decoder's
// recovered originals do (with `corrupt`, every third solve gets non-zero
// bytes past one row's length: inconsistent recovery data), forms the rows
// R = L U X the sweeps invert, and runs the sweeps and the vector product on
// copies of them.  stats[0]: bytes of the rows (and result words [0..m])
// where the vector product's outcome differs from the sweeps'; stats[2]:
// solves it flagged for the sweeps (stats[1] and stats[3] read zero: no
// second product path is built).  Returns 0 when the product matches the
// sweeps, 1 when not, -1 on a device error.
extern "C" __attribute__((visibility("default"))) int sgpu_selftest_solve_paths(uint32_t seed, uint32_t nsolves,
                                                                                uint32_t corrupt,
                                                                                uint32_t* stats)
{
    if (nsolves == 0 || !gf_init())
        return -1;
    bind_device();
    uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() -> uint32_t {
        st ^= st << 13;
        st ^= st >> 7;
        st ^= st << 17;
        return (uint32_t)(st >> 16);
    };
    struct Sys
    {
        uint32_t m, maxB, rowBase, coefOff, result;
        std::vector<uint8_t> C, R;   // C[j*m + i]; rows of maxB bytes
    };
    std::vector<Sys> sys(nsolves);
    uint32_t rows = 0, coefBytes = 0, resWords = 0, maxRows = 0;
    for (uint32_t s = 0; s < nsolves; ++s) {
        Sys& y = sys[s];
        // (every row count the product solves take: 16..120, so every
        // rows-per-wave variant of k_solve_tr runs)
        y.m = 16 + rnd() % (kProductMaxRows - 15);
        static const uint32_t kLens[6] = {1402, 600, 1100, 2000, 4100, 6000};
        y.maxB = kLens[rnd() % 6];
        y.rowBase = rows;
        y.coefOff = coefBytes;
        y.result = resWords;
        rows += y.m;
        coefBytes += (y.m * y.m + 15u) & ~15u;
        resWords += y.m + 2;
        maxRows = std::max(maxRows, y.m);
        const uint32_t m = y.m, B = y.maxB;
        y.C.resize(m * m);
        for (uint32_t k = 0; k < m * m; ++k)
            y.C[k] = (rnd() % 8) ? (uint8_t)rnd() : 0;
        for (uint32_t i = 0; i < m; ++i)
            if (!y.C[i * m + i])
                y.C[i * m + i] = 1 + rnd() % 255;
        // the true rows: a length prefix, bytes up to the length, zeros after
        std::vector<uint8_t> X((size_t)m * B, 0);
        for (uint32_t i = 0; i < m; ++i) {
            uint8_t* x = &X[(size_t)i * B];
            uint32_t b;
            if (rnd() % 4 == 0) {
                const uint32_t len = 1 + rnd() % 100;   // one-byte prefix
                x[0] = (uint8_t)len;
                b = 1 + len;
            } else {
                const uint32_t len = 128 + rnd() % (B - 130);   // two-byte prefix
                x[0] = (uint8_t)(0x80 | (len >> 8));
                x[1] = (uint8_t)len;
                b = 2 + len;
            }
            for (uint32_t p = (x[0] & 0x80) ? 2 : 1; p < b; ++p)
                x[p] = (uint8_t)rnd();
            if (corrupt && s % 3 == 0 && i == m / 2 && b < B)
                for (unsigned k = 0; k < 3; ++k)
                    x[b + rnd() % (B - b)] = 1 + rnd() % 255;
        }
        // y = U x (upper part with the diagonal), then R = L y (unit lower)
        std::vector<uint8_t> Y((size_t)m * B, 0);
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t i = j; i < m; ++i)
                if (const uint8_t c = y.C[j * m + i])
                    for (uint32_t p = 0; p < B; ++p)
                        Y[(size_t)j * B + p] ^= gf_mul(X[(size_t)i * B + p], c);
        y.R = Y;
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t i = 0; i < j; ++i)
                if (const uint8_t c = y.C[j * m + i])
                    for (uint32_t p = 0; p < B; ++p)
                        y.R[(size_t)j * B + p] ^= gf_mul(Y[(size_t)i * B + p], c);
    }
    // device layout: row buffers of 6 KiB + 2 KiB slack, coefficients,
    // results, heads, scratch, descriptors, items
    constexpr uint32_t kRowCap = 8192;
    std::vector<SolveItem> items;
    std::vector<SolveDesc> descs(nsolves);
    std::vector<SolveRow> rdesc(rows);
    uint64_t scratch = 0;
    for (uint32_t s = 0; s < nsolves; ++s) {
        const Sys& y = sys[s];
        for (uint32_t t = 0; t < y.maxB; t += solve_tile_bytes(y.m))
            items.push_back(SolveItem{s, t});
        scratch += solve_t_bytes(y.m) + ((solve_x_bytes(y.m, y.maxB) + 255u) & ~(uint64_t)255u);
    }
    uint8_t *dRows = nullptr, *dCoef = nullptr, *dHead = nullptr, *dScratch = nullptr;
    uint32_t* dRes = nullptr;
    SolveDesc* dDesc = nullptr;
    SolveRow* dRowD = nullptr;
    SolveItem* dItems = nullptr;
    uint64_t* dAcct = nullptr;
    bool ok = hipMalloc(&dRows, (size_t)rows * kRowCap) == hipSuccess &&
              hipMalloc(&dCoef, coefBytes) == hipSuccess && hipMalloc(&dHead, (size_t)rows * 16) == hipSuccess &&
              hipMalloc(&dScratch, scratch + 256) == hipSuccess &&
              hipMalloc(&dRes, (size_t)resWords * 4) == hipSuccess &&
              hipMalloc(&dDesc, nsolves * sizeof(SolveDesc)) == hipSuccess &&
              hipMalloc(&dRowD, rows * sizeof(SolveRow)) == hipSuccess &&
              hipMalloc(&dItems, items.size() * sizeof(SolveItem)) == hipSuccess &&
              hipMalloc(&dAcct, 4 * sizeof(uint64_t)) == hipSuccess;
    std::vector<uint8_t> hostRows((size_t)rows * kRowCap, 0), hostHead((size_t)rows * 16, 0);
    std::vector<uint8_t> hostCoef(coefBytes, 0);
    if (ok) {
        uint64_t sc = (uint64_t)(uintptr_t)dScratch;
        for (uint32_t s = 0; s < nsolves; ++s) {
            const Sys& y = sys[s];
            SolveDesc& d = descs[s];
            std::memset(&d, 0, sizeof(d));
            d.m = y.m;
            d.rowBegin = y.rowBase;
            d.coefOffset = y.coefOff;
            d.result = y.result;
            d.maxBytes = y.maxB;
            d.head = (uint64_t)(uintptr_t)(dHead + (size_t)y.rowBase * 16);
            d.tinv = sc;
            sc += solve_t_bytes(y.m);
            d.xout = sc;
            sc += (solve_x_bytes(y.m, y.maxB) + 255u) & ~(uint64_t)255u;
            std::memcpy(&hostCoef[y.coefOff], y.C.data(), y.m * y.m);
            for (uint32_t j = 0; j < y.m; ++j) {
                const uint32_t r = y.rowBase + j;
                std::memcpy(&hostRows[(size_t)r * kRowCap], &y.R[(size_t)j * y.maxB], y.maxB);
                std::memcpy(&hostHead[(size_t)r * 16], &y.R[(size_t)j * y.maxB], 16);
                SolveRow& w = rdesc[r];
                std::memset(&w, 0, sizeof(w));
                w.buf = (uint64_t)(uintptr_t)(dRows + (size_t)r * kRowCap);
                w.initBytes = w.lowerLen = w.finalBytes = y.maxB;
            }
        }
        ok = hipMemcpy(dCoef, hostCoef.data(), coefBytes, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(dHead, hostHead.data(), hostHead.size(), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(dDesc, descs.data(), nsolves * sizeof(SolveDesc), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(dRowD, rdesc.data(), rows * sizeof(SolveRow), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(dItems, items.data(), items.size() * sizeof(SolveItem), hipMemcpyHostToDevice) == hipSuccess;
    }
    std::vector<uint8_t> outRows[2];
    std::vector<uint32_t> outRes[2];
    const SolvePath paths[2] = {kPathSweeps, kPathVector};
    for (int k = 0; k < 2 && ok; ++k) {
        // (on the solve's own stream: a plain hipMemset runs on the null
        // stream, which does not order against g_stream (non-blocking), and a
        // late scratch fill overwrote some T inverses mid-solve)
        ok = hipMemcpyAsync(dRows, hostRows.data(), hostRows.size(), hipMemcpyHostToDevice, g_stream) == hipSuccess &&
             hipMemsetAsync(dRes, 0xff, (size_t)resWords * 4, g_stream) == hipSuccess &&
             hipMemsetAsync(dScratch, 0xa5, scratch + 256, g_stream) == hipSuccess &&
             hipMemsetAsync(dAcct, 0, 4 * sizeof(uint64_t), g_stream) == hipSuccess;
        if (!ok)
            break;
        launch_solve(dDesc, dRowD, dCoef, dRes, dItems, (uint32_t)items.size(), maxRows, dAcct, 0, nsolves,
                     paths[k]);
        outRows[k].resize(hostRows.size());
        outRes[k].resize(resWords);
        ok = hipStreamSynchronize(g_stream) == hipSuccess &&
             hipMemcpy(outRows[k].data(), dRows, hostRows.size(), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(outRes[k].data(), dRes, (size_t)resWords * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(dRows);
    (void)hipFree(dCoef);
    (void)hipFree(dHead);
    (void)hipFree(dScratch);
    (void)hipFree(dRes);
    (void)hipFree(dDesc);
    (void)hipFree(dRowD);
    (void)hipFree(dItems);
    (void)hipFree(dAcct);
    if (!ok)
        return -1;
    uint32_t diff[2] = {0, 0}, flagged[2] = {0, 0};   // [1]: a second product path (none since round 5)
    for (int k = 1; k < 2; ++k) {
        for (size_t b = 0; b < hostRows.size(); ++b)
            diff[k - 1] += outRows[k][b] != outRows[0][b];
        for (uint32_t s = 0; s < nsolves; ++s) {
            const Sys& y = sys[s];
            for (uint32_t w = 0; w <= y.m; ++w)
                diff[k - 1] += outRes[k][y.result + w] != outRes[0][y.result + w];
            flagged[k - 1] += outRes[k][y.result + y.m + 1] != 0;
        }
    }
    if (stats) {
        stats[0] = diff[0];
        stats[1] = diff[1];
        stats[2] = flagged[0];
        stats[3] = flagged[1];
    }
    return (diff[0] || diff[1]) ? 1 : 0;
}


void* be_stage_h2d(void* dst, const void* src, size_t bytes)
{
    bind_device();
    hipEvent_t e = nullptr;
    {
        std::lock_guard<std::mutex> g(g_evMu);
        if (!g_fenceFree.empty()) {
            e = g_fenceFree.back();
            g_fenceFree.pop_back();
        }
    }
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
        return nullptr;
    // (a copy-engine copy: staging it by a kernel reading mapped pinned
    // memory slowed the codec kernels beside it)
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g_stageStream) != hipSuccess)
        return nullptr;
    if (hipEventRecord(e, g_stageStream) != hipSuccess)
        return nullptr;
    return e;
}

void be_wait_mark(void* mark)
{
    bind_device();
    if (mark)
        check(hipStreamWaitEvent(g_stream, static_cast<hipEvent_t>(mark), 0), "hipStreamWaitEvent");
}

void be_mark_release(void* mark)
{
    if (!mark)
        return;
    std::lock_guard<std::mutex> g(g_evMu);
    g_fenceFree.push_back(static_cast<hipEvent_t>(mark));
}

hipEvent_t take_mark()
{
    hipEvent_t e = nullptr;
    {
        std::lock_guard<std::mutex> g(g_evMu);
        if (!g_fenceFree.empty()) {
            e = g_fenceFree.back();
            g_fenceFree.pop_back();
        }
    }
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
        return nullptr;
    return e;
}

bool be_gather(const IngestDesc* descsHost, void* descsDev, uint32_t count, const void* devStage,
               void* hostOut, size_t bytes, void** packed, void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    uint32_t maxBytes = 0;
    for (uint32_t i = 0; i < count; ++i)
        maxBytes = std::max(maxBytes, descsHost[i].bytes + descsHost[i].hdrLen);
    const uint32_t gatherChunks = maxBytes ? (maxBytes + kIngestChunkBytes - 1) / kIngestChunkBytes : 1;
    if (hipMemcpyAsync(descsDev, descsHost, (size_t)count * sizeof(IngestDesc), hipMemcpyHostToDevice,
                       g_gatherStream) != hipSuccess)
        return false;
    hipLaunchKernelGGL(k_ingest, dim3((count + kIngestWaves - 1) / kIngestWaves, gatherChunks),
                       dim3(64 * kIngestWaves), 0, g_gatherStream, static_cast<const IngestDesc*>(descsDev), count,
                       (const uint32_t*)nullptr);
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    if (hipMemcpyAsync(hostOut, devStage, bytes, hipMemcpyDeviceToHost, g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_scan_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, void* devStage,
                  void* hostOut, void** packed, void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    {
        Timed t(kBeScan, g_gatherStream);
        hipLaunchKernelGGL(k_scan, dim3((count + kScanThreads - 1) / kScanThreads), dim3(kScanThreads), 0,
                           g_gatherStream, (uint64_t)(uintptr_t)rows, stride, lens, count,
                           (uint64_t)(uintptr_t)devStage);
    }
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    if (hipMemcpyAsync(hostOut, devStage, (size_t)count * sizeof(RowHead), hipMemcpyDeviceToHost,
                       g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_walk_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, uint32_t maxFrames,
                  void* devStage, void* hostOut, void** packed, void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    {
        Timed t(kBeWalk, g_gatherStream);
        hipLaunchKernelGGL(k_walk, dim3((count + kWalkThreads - 1) / kWalkThreads), dim3(kWalkThreads), 0,
                           g_gatherStream, (uint64_t)(uintptr_t)rows, stride, lens, count, maxFrames,
                           (uint64_t)(uintptr_t)devStage);
    }
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    if (hipMemcpyAsync(hostOut, devStage, (size_t)packed_bytes(count, maxFrames), hipMemcpyDeviceToHost,
                       g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_dense_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, uint32_t maxFrames,
                   uint32_t maxRecords, void* devStage, void* hostOut, void** packed, void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    const uint64_t out = (uint64_t)(uintptr_t)devStage;
    const uint64_t scratch = out + dense_scratch_offset(count, maxRecords);
    {
        Timed t(kBeWalk, g_gatherStream);
        hipLaunchKernelGGL(k_walkd, dim3((count + kWalkThreads - 1) / kWalkThreads), dim3(kWalkThreads), 0,
                           g_gatherStream, (uint64_t)(uintptr_t)rows, stride, lens, count, maxFrames, scratch,
                           out + 16);
    }
    // (the rows have been read: what follows works on the staging area alone)
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    {
        Timed t(kBeRowsum, g_gatherStream);
        hipLaunchKernelGGL(k_rowsum, dim3(1), dim3(kRowsumThreads), 0, g_gatherStream, out, count, maxFrames,
                           maxRecords);
    }
    {
        Timed t(kBeCompact, g_gatherStream);
        const uint64_t lanes = 2 * (uint64_t)maxRecords;
        hipLaunchKernelGGL(k_compact, dim3((uint32_t)((lanes + kCompactThreads - 1) / kCompactThreads)),
                           dim3(kCompactThreads), 0, g_gatherStream, out, scratch, count, maxFrames, maxRecords);
    }
    if (hipMemcpyAsync(hostOut, devStage, (size_t)dense_bytes(count, maxRecords), hipMemcpyDeviceToHost,
                       g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_stream_rows(const void* rows, uint64_t stride, const uint32_t* starts, const uint32_t* ends, uint32_t count,
                    uint32_t maxFrames, uint32_t maxRecords, void* devStage, void* hostOut, void** packed,
                    void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    const uint64_t out = (uint64_t)(uintptr_t)devStage;
    const uint64_t scratch = out + streams_scratch_offset(count, maxRecords);
    {
        Timed t(kBeStreamWalk, g_gatherStream);
        hipLaunchKernelGGL(k_streamwalk, dim3((count + kStreamWaves - 1) / kStreamWaves), dim3(kStreamWalkThreads), 0,
                           g_gatherStream, (uint64_t)(uintptr_t)rows, stride, starts, ends, count, maxFrames, scratch,
                           out + 16, out + streams_next_offset(count, maxRecords));
    }
    // (the rows have been read: what follows works on the staging area alone)
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    {
        Timed t(kBeRowsum, g_gatherStream);
        hipLaunchKernelGGL(k_rowsum, dim3(1), dim3(kRowsumThreads), 0, g_gatherStream, out, count, maxFrames,
                           maxRecords);
    }
    {
        Timed t(kBeCompact, g_gatherStream);
        const uint64_t lanes = 2 * (uint64_t)maxRecords;
        hipLaunchKernelGGL(k_compact, dim3((uint32_t)((lanes + kCompactThreads - 1) / kCompactThreads)),
                           dim3(kCompactThreads), 0, g_gatherStream, out, scratch, count, maxFrames, maxRecords);
    }
    if (hipMemcpyAsync(hostOut, devStage, (size_t)streams_bytes(count, maxRecords), hipMemcpyDeviceToHost,
                       g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_ackwalk_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count, uint32_t maxFrames,
                     uint32_t ackSlots, uint32_t ackBytes, void* devStage, void* hostOut, void** packed,
                     void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    {
        Timed t(kBeAckWalk, g_gatherStream);
        hipLaunchKernelGGL(k_ackwalk, dim3((count + kAckWalkThreads - 1) / kAckWalkThreads), dim3(kAckWalkThreads), 0,
                           g_gatherStream, (uint64_t)(uintptr_t)rows, stride, lens, count, maxFrames, ackSlots,
                           ackBytes, (uint64_t)(uintptr_t)devStage,
                           (uint64_t)(uintptr_t)devStage + duplex_slots_offset(count, maxFrames));
    }
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    if (hipMemcpyAsync(hostOut, devStage, (size_t)duplex_bytes(count, maxFrames, ackSlots, ackBytes),
                       hipMemcpyDeviceToHost, g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_duplex_dense_rows(const void* rows, uint64_t stride, const uint32_t* lens, uint32_t count,
                          uint32_t maxFrames, uint32_t ackSlots, uint32_t ackBytes, uint32_t maxRecords,
                          uint32_t maxAcks, void* devStage, void* hostOut, void** packed, void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    const uint64_t out = (uint64_t)(uintptr_t)devStage;
    const uint64_t recs = out + duplex_dense_scratch_records(count, maxRecords, maxAcks, ackBytes);
    const uint64_t slots = out + duplex_dense_scratch_slots(count, maxFrames, maxRecords, maxAcks, ackBytes);
    const uint64_t counts =
        out + duplex_dense_scratch_counts(count, maxFrames, ackSlots, maxRecords, maxAcks, ackBytes);
    {
        Timed t(kBeAckWalk, g_gatherStream);
        hipLaunchKernelGGL(k_ackwalkd, dim3((count + kAckWalkdThreads - 1) / kAckWalkdThreads),
                           dim3(kAckWalkdThreads), 0, g_gatherStream, (uint64_t)(uintptr_t)rows, stride, lens, count,
                           maxFrames, ackSlots, ackBytes, recs, slots, counts, out + 16);
    }
    // (the rows have been read: what follows works on the staging area alone)
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    {
        Timed t(kBeRowsum2, g_gatherStream);
        hipLaunchKernelGGL(k_rowsum2, dim3(1), dim3(kRowsum2Threads), 0, g_gatherStream, out, counts, count,
                           maxFrames, ackSlots, maxRecords, maxAcks);
    }
    {
        Timed t(kBeCompact, g_gatherStream);
        const uint64_t lanes = 2 * (uint64_t)maxRecords;
        hipLaunchKernelGGL(k_compact, dim3((uint32_t)((lanes + kCompactThreads - 1) / kCompactThreads)),
                           dim3(kCompactThreads), 0, g_gatherStream, out, recs, count, maxFrames, maxRecords);
    }
    {
        Timed t(kBeSlots, g_gatherStream);
        const uint64_t lanes = (uint64_t)maxAcks * (ackBytes >> 4);
        hipLaunchKernelGGL(k_slots, dim3((uint32_t)((lanes + kSlotsThreads - 1) / kSlotsThreads)),
                           dim3(kSlotsThreads), 0, g_gatherStream, out, slots, count, ackSlots, ackBytes, maxRecords,
                           maxAcks);
    }
    if (hipMemcpyAsync(hostOut, devStage, (size_t)duplex_dense_bytes(count, maxRecords, maxAcks, ackBytes),
                       hipMemcpyDeviceToHost, g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_duplex_stream_rows(const void* rows, uint64_t stride, const uint32_t* starts, const uint32_t* ends,
                           uint32_t count, uint32_t maxFrames, uint32_t ackSlots, uint32_t ackBytes,
                           uint32_t maxRecords, uint32_t maxAcks, void* devStage, void* hostOut, void** packed,
                           void** landed)
{
    bind_device();
    *packed = *landed = nullptr;
    hipEvent_t p = take_mark(), l = take_mark();
    if (!p || !l) {
        be_mark_release(p);
        be_mark_release(l);
        return false;
    }
    const uint64_t out = (uint64_t)(uintptr_t)devStage;
    const uint64_t recs = out + duplex_streams_scratch_records(count, maxRecords, maxAcks, ackBytes);
    const uint64_t slots = out + duplex_streams_scratch_slots(count, maxFrames, maxRecords, maxAcks, ackBytes);
    const uint64_t counts =
        out + duplex_streams_scratch_counts(count, maxFrames, ackSlots, maxRecords, maxAcks, ackBytes);
    {
        Timed t(kBeAckStreamWalk, g_gatherStream);
        hipLaunchKernelGGL(k_ackstreamwalk, dim3((count + kAckStreamWalkThreads - 1) / kAckStreamWalkThreads),
                           dim3(kAckStreamWalkThreads), 0, g_gatherStream, (uint64_t)(uintptr_t)rows, stride, starts,
                           ends, count, maxFrames, ackSlots, ackBytes, recs, slots, counts, out + 16,
                           out + duplex_streams_next_offset(count, maxRecords, maxAcks, ackBytes));
    }
    // (the rows have been read: what follows works on the staging area alone)
    if (hipEventRecord(p, g_gatherStream) != hipSuccess)
        return false;
    *packed = p;
    {
        Timed t(kBeRowsum2, g_gatherStream);
        hipLaunchKernelGGL(k_rowsum2, dim3(1), dim3(kRowsum2Threads), 0, g_gatherStream, out, counts, count,
                           maxFrames, ackSlots, maxRecords, maxAcks);
    }
    {
        Timed t(kBeCompact, g_gatherStream);
        const uint64_t lanes = 2 * (uint64_t)maxRecords;
        hipLaunchKernelGGL(k_compact, dim3((uint32_t)((lanes + kCompactThreads - 1) / kCompactThreads)),
                           dim3(kCompactThreads), 0, g_gatherStream, out, recs, count, maxFrames, maxRecords);
    }
    {
        Timed t(kBeSlots, g_gatherStream);
        const uint64_t lanes = (uint64_t)maxAcks * (ackBytes >> 4);
        hipLaunchKernelGGL(k_slots, dim3((uint32_t)((lanes + kSlotsThreads - 1) / kSlotsThreads)),
                           dim3(kSlotsThreads), 0, g_gatherStream, out, slots, count, ackSlots, ackBytes, maxRecords,
                           maxAcks);
    }
    if (hipMemcpyAsync(hostOut, devStage, (size_t)duplex_streams_bytes(count, maxRecords, maxAcks, ackBytes),
                       hipMemcpyDeviceToHost, g_gatherStream) != hipSuccess ||
        hipEventRecord(l, g_gatherStream) != hipSuccess) {
        be_mark_release(l);
        return false;
    }
    *landed = l;
    return true;
}

bool be_mark_sync(void* mark)
{
    bind_device();
    if (!mark)
        return false;
    const hipError_t e = hipEventSynchronize(static_cast<hipEvent_t>(mark));
    be_mark_release(mark);
    if (g_timing && e == hipSuccess)   // (a scan kernel's bracket ends before its landed mark)
        harvest_timing(false);
    if (e != hipSuccess) {
        check(e, "hipEventSynchronize(mark)");
        return false;
    }
    return true;
}

bool be_sync()
{
    bind_device();
    const hipError_t e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) {
        check(e, "hipStreamSynchronize");
        return false;
    }
    harvest_timing(true);
    return true;
}

void* be_fence()
{
    bind_device();
    hipEvent_t e = nullptr;
    {
        std::lock_guard<std::mutex> g(g_evMu);
        if (!g_fenceFree.empty()) {
            e = g_fenceFree.back();
            g_fenceFree.pop_back();
        }
    }
    if (!e && hipEventCreateWithFlags(&e, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess)
        return nullptr;
    if (hipEventRecord(e, g_stream) != hipSuccess)
        return nullptr;
    return e;
}

bool be_fence_wait(void* fence, unsigned spinUs, bool sleepPoll)
{
    bind_device();
    if (!fence)
        return false;
    hipEvent_t e = static_cast<hipEvent_t>(fence);
    // Poll first: a blocking-sync wait sleeps until an interrupt wakes the
    // thread, tens of microseconds a flush on the latency-bound single-stream
    // path (C3); the completer is a dedicated thread, so for small flushes it
    // spins up to spinUs before it sleeps (large ones leave the core to the
    // application's threads).
    const int64_t kFenceSpinUs = spinUs;
    hipError_t r = hipEventQuery(e);
    if (r == hipErrorNotReady && kFenceSpinUs > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        do {
            __builtin_ia32_pause();
            r = hipEventQuery(e);
        } while (r == hipErrorNotReady &&
                 std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0)
                         .count() < kFenceSpinUs);
    }
    // Large flushes: poll with short sleeps instead of hipEventSynchronize,
    // whose runtime spins up to ~200 us on the core before it blocks -- CPU
    // time the process's quota (16 CPUs on the box, every one of them busy
    // on the headline) takes from the stepping threads.  A poll every
    // 10-40 us costs a few us of CPU per fence and at most one interval of
    // latency on a completion that is ~0.4 ms away.
    if (r == hipErrorNotReady && sleepPoll) {
        long ns = 10000;
        do {
            struct timespec ts = {0, ns};
            nanosleep(&ts, nullptr);
            if (ns < 40000)
                ns += 10000;
            r = hipEventQuery(e);
        } while (r == hipErrorNotReady);
    }
    if (r == hipErrorNotReady)
        r = hipEventSynchronize(e);
    if (r != hipSuccess) {
        check(r, "hipEventSynchronize");
        return false;
    }
    harvest_timing(false);
    std::lock_guard<std::mutex> g(g_evMu);
    g_fenceFree.push_back(e);
    return true;
}

void be_timing_enable(bool on)
{
    g_timing = on;
}
double be_timing_kernel_ms(BeKernel kind)
{
    return kind < kBeKernelKinds ? g_kernelMs[kind] : 0.0;
}

void be_timing_reset()
{
    for (double& v : g_kernelMs)
        v = 0;
    g_totalMs = 0;
}
double be_timing_total_ms() { return g_totalMs; }

} // namespace sgpu
