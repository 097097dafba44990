// gc_zstd_lz.hip -- K1: all-positions-parallel match finder + deterministic greedy/lazy parse.
//
// Replaces, for one <=128 KiB zstd block per workgroup, the serial per-position loop of
// ZSTD_compressBlock_doubleFast_noDict_generic (C/zstd/zstd_double_fast.c:105-323) and the sequence store
// (ZSTD_storeSeq, zstd_compress_internal.h:776).  The CPU loop visits one position at a time and skips the
// inside of matches; a CDNA4 workgroup instead evaluates a chunk of LZ_T consecutive positions at once:
//
//   P0  every lane loads the 8 bytes at its position and hashes them twice: a 5-byte "short" hash and an
//       8-byte "long" hash (the reference's two-table idea, zstd_double_fast.c:132-141; the hash functions
//       themselves are free choices and use 32-bit multiplies, which are full rate on the VALU)
//   P1  probe both LDS tables (entry = position<<15 | 15-bit tag, so hash collisions are rejected from the
//       tag alone without touching memory)
//   P2  insert: ds_max_u32 -> "most recent position wins", identical to sequential insertion order, hence
//       the result does not depend on wave timing (the encoder is deterministic)
//   P3  a small generation-stamped table (ds_min_u32 -> first occurrence inside the chunk) supplies the
//       short-distance candidates that P1 cannot see because the whole chunk was probed before it was inserted
//   P4  candidates are verified against the immutable input: all candidate windows (16 B each) are requested
//       together so only one memory latency is exposed; a saturated best candidate is extended 16 B per round
//       up to GC_MATCH_CAP; longer matches appear as chains of capped matches with equal offset, merged in K3
//   P5  parse: next(t) = t+len if a match is taken at t, else t+1.  Each wave resolves its 64-position
//       segment for EVERY possible entry lane by pointer doubling through ds_bpermute (6 rounds), one lane
//       chains the 16 wave exits, then each wave marks its real path by binary lifting over the same jump tables.
//   P6  emit: wave ballots + popcounts place literals and sequences; no atomics, order = position order.
//
// LDS: 64 KiB long table + 64 KiB short table + 8 KiB chunk table + 8 KiB parse scratch (1 workgroup / CU).
#include "gc_lz_parse.h"
#include "gpucodec.h"      // gc_batch_item

#define LZ_LOG_L    14u              // long-hash table: 2^14 entries
#define LZ_LOG_S    14u              // short-hash table
#define LZ_LOG_C    11u              // chunk-local table
#define LZ_TAG_BITS 15u

// ---- dictionaries (gpucodec.h "ZSTD, dictionaries")
#define LZ_LOG_DICT GC_ZDICT_LOG     // the dictionary's two digest tables: 2^17 entries each (global memory, 2 x 512 KiB, L2-resident); index + tag use all 32 hash bits
// entry = (dictionary position + 1) << 15 | 15-bit tag; 0 = empty.  Positions + 1 stay below 2^17 (GC_ZSTD_DICT_MAX = 128 KiB)
struct LzDict {
    const uint8_t* bytes = nullptr;  // size bytes, then at least 32 bytes of zeros (a 16-byte compare window behind the last byte stays inside the allocation)
    const uint32_t* tabL = nullptr;
    const uint32_t* tabS = nullptr;
    uint32_t size = 0;
    uint32_t* sTail = nullptr;       // LDS, GC_MATCH_CAP words: the records the previous step of LZ_T positions ended with (P4b)
};

// 16 bytes at src[pos..] of which only those in front of `end` are read; the rest come out as zeros
__device__ __forceinline__ LzW16 lz_ld16_end(const uint8_t* src, uint64_t pos, uint64_t end)
{
    if (pos + 16u <= end) return lz_ld16(src, pos);
    LzW16 w; w.a = 0; w.b = 0;
    for (uint32_t k = 0; k < 8u; k++)  if (pos + k < end) w.a |= (uint64_t)src[pos + k] << (8u * k);
    for (uint32_t k = 8u; k < 16u; k++) if (pos + k < end) w.b |= (uint64_t)src[pos + k] << (8u * (k - 8u));
    return w;
}

// P4 with a dictionary: up to three candidates inside the block (as lz_verify, but no window is read across the block's readable end wEnd, relative to wsrc)
// and up to two in the dictionary (q0 / q1: dictionary position + 1, 0 = none), all five windows requested together.  A dictionary match is cut at the
// dictionary's end; its offset is pw + (D.size - position).  Ties go to the candidate looked at first: block candidates, then the dictionary's.
__device__ __forceinline__ void lz_verify_dict(const uint8_t* wsrc, uint32_t wEnd, uint32_t pw, const LzW16& me, const uint32_t cand[3], int nc,
                                               const LzDict& D, uint32_t q0, uint32_t q1, uint32_t maxLen, uint32_t& bestLen, uint32_t& bestOff)
{
    int bestGain = -1000;
    LzW16 cw[3], dw0, dw1;
    for (int i = 0; i < 3; i++) if (i < nc) cw[i] = lz_ld16_end(wsrc, cand[i], wEnd);
    dw0.a = dw0.b = dw1.a = dw1.b = 0;
    if (q0) dw0 = lz_ld16(D.bytes, q0 - 1u);
    if (q1) dw1 = lz_ld16(D.bytes, q1 - 1u);
    uint32_t bestC = 0, bestMax = maxLen; bool inDict = false;
    for (int i = 0; i < 3; i++) {
        if (i < nc) {
            uint32_t len = lz_cmp16(me, cw[i]);
            if (len > maxLen) len = maxLen;
            if (len >= GC_MIN_MATCH) {
                int g = lz_gain(len, pw - cand[i]);
                if (g > bestGain) { bestGain = g; bestLen = len; bestOff = pw - cand[i]; bestC = cand[i]; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t q = i ? q1 : q0;
        if (q) {
            const uint32_t dpos = q - 1u, room = D.size - dpos, lim = room < maxLen ? room : maxLen;
            uint32_t len = lz_cmp16(me, i ? dw1 : dw0);
            if (len > lim) len = lim;
            if (len >= GC_MIN_MATCH) {
                const uint32_t off = pw + room;
                int g = lz_gain(len, off);
                if (g > bestGain) { bestGain = g; bestLen = len; bestOff = off; bestC = dpos; bestMax = lim; inDict = true; }
            }
        }
    }
    while (bestLen >= 16u && (bestLen & 15u) == 0u && bestLen < bestMax) {
        LzW16 x = lz_ld16_end(wsrc, (uint64_t)pw + bestLen, wEnd);
        LzW16 y = inDict ? lz_ld16(D.bytes, (uint64_t)bestC + bestLen) : lz_ld16_end(wsrc, (uint64_t)bestC + bestLen, wEnd);
        uint32_t more = lz_cmp16(x, y);
        bestLen += more;
        if (bestLen > bestMax) bestLen = bestMax;
        if (more < 16u) break;
    }
}

// length (0 .. maxLen) of the match at offset `off` for position pw: its source lies in the block (off <= pw) or starts in the dictionary, where it is cut at the
// dictionary's end.  off <= pw + D.size.
__device__ __forceinline__ uint32_t lz_len_at(const uint8_t* wsrc, uint32_t wEnd, uint32_t pw, const LzW16& me, uint32_t off, const LzDict& D, uint32_t maxLen)
{
    const bool inDict = off > pw;
    uint32_t lim = maxLen, c = pw - off;
    if (inDict) {
        const uint32_t back = off - pw;
        if (back > D.size) return 0u;
        c = D.size - back;
        if (back < lim) lim = back;
    }
    uint32_t len = lz_cmp16(me, inDict ? lz_ld16(D.bytes, c) : lz_ld16_end(wsrc, c, wEnd));
    if (len > lim) len = lim;
    while (len >= 16u && (len & 15u) == 0u && len < lim) {
        const LzW16 x = lz_ld16_end(wsrc, (uint64_t)pw + len, wEnd);
        const LzW16 y = inDict ? lz_ld16(D.bytes, (uint64_t)c + len) : lz_ld16_end(wsrc, (uint64_t)c + len, wEnd);
        const uint32_t more = lz_cmp16(x, y);
        len += more;
        if (len > lim) len = lim;
        if (more < 16u) break;
    }
    return len;
}

// One block: bytes [base, base + n) of src; `end` is where the readable input ends for this block (the end of the whole stream for K1, the end of the
// item for K1b): no byte at or behind src + end is read, and a position takes part in matching only if GC_MATCH_CAP + 16 bytes lie in front of `end`.
// The LDS tables belong to the calling kernel (the same four for K1 and K1b: the matches depend on their geometry).
//
// DICT (K1b with a dictionary, DESIGN.md section 4 "Dictionaries"): D.bytes lie as history immediately in front of the block.  Beside the LDS probe every position
// probes the dictionary's two digest tables in global memory (read-only, shared by all workgroups) and verifies up to two more candidates against the dictionary
// in the same memory round trip; a dictionary match at dictionary position q has offset p + (D.size - q) and is cut at the dictionary's end.  Small items are the
// point of a dictionary, so this variant lets every position with 8 bytes in front of the block's end take part: windows that would cross `end` are read byte
// by byte (lz_ld16_end), never behind it.
template <bool DICT>
__device__ __forceinline__ void lz_block(const uint8_t* __restrict__ src, const uint64_t base, const uint32_t n, const uint64_t end,
                                         GcSeqRaw* __restrict__ mySeq, uint8_t* __restrict__ myLit, GcBlockMeta* __restrict__ myMeta,
                                         unsigned long long* __restrict__ prof,
                                         uint32_t (&tabL)[1u << LZ_LOG_L], uint32_t (&tabS)[1u << LZ_LOG_S], uint32_t (&tabC)[1u << LZ_LOG_C], LzParseLds& S,
                                         const LzDict D = LzDict())
{
    const uint32_t t = threadIdx.x;

    for (uint32_t i = t; i < (1u << LZ_LOG_L); i += LZ_T) tabL[i] = 0;
    for (uint32_t i = t; i < (1u << LZ_LOG_S); i += LZ_T) tabS[i] = 0;
    for (uint32_t i = t; i < (1u << LZ_LOG_C); i += LZ_T) tabC[i] = 0xFFFFFFFFu;
    if (t == 0) S.sCursor = 0;
    if constexpr (DICT) if (t < GC_MATCH_CAP) D.sTail[t] = 0;
    __syncthreads();

    LzProf P; P.on = prof != nullptr; for (int i = 0; i < GC_LZ_PHASES; i++) P.pc[i] = 0;
    P.tprev = P.on ? gc_clock() : 0ull;
    uint32_t totalSeq = 0, totalLit = 0;   // uniform running totals
    const uint32_t nChunks = (n + LZ_T - 1) / LZ_T;
    LzW16 own; own.a = 0; own.b = 0;                    // own 16 bytes, always loaded one chunk ahead
    if constexpr (DICT) { if (t < n) own = lz_ld16_end(src, base + t, end); }
    else if (base + t + GC_MATCH_CAP + 16u <= end) own = lz_ld16(src, base + t);

    for (uint32_t k = 0; k < nChunks; k++) {
        const uint32_t cbase = k * LZ_T;
        const uint32_t p = cbase + t;
        const bool inBlock = p < n;
        // positions closer than 8 bytes to the block end, or without a readable compare window, stay literals
        const bool canHash = p + 8u <= n && (DICT || base + p + GC_MATCH_CAP + 16u <= end);

        // ---- P0/P1: load, hash, probe
        uint32_t lo = 0, hi = 0, hL = 0, hS = 0, eL = 0, eS = 0;
        const LzW16 me = own;
        if (canHash) {
            lo = (uint32_t)me.a; hi = (uint32_t)(me.a >> 32);
            hL = lz_hash_long(lo, hi); hS = lz_hash_short(lo, hi);
            eL = tabL[hL >> (32u - LZ_LOG_L)];
            eS = tabS[hS >> (32u - LZ_LOG_S)];
        }
        uint32_t dL = 0, dS = 0;                              // the dictionary's entries for the same two hashes (requested here, used in P4)
        if constexpr (DICT) if (canHash) { dL = D.tabL[hL >> (32u - LZ_LOG_DICT)]; dS = D.tabS[hS >> (32u - LZ_LOG_DICT)]; }
        const uint32_t tagL = (hL >> (32u - LZ_LOG_L - LZ_TAG_BITS)) & ((1u << LZ_TAG_BITS) - 1u);
        const uint32_t tagS = (hS >> (32u - LZ_LOG_S - LZ_TAG_BITS)) & ((1u << LZ_TAG_BITS) - 1u);
        const uint32_t gen = (~k) & 0xFFu;
        const uint32_t tagC = (hS >> 4) & 0x3FFFu;
        const uint32_t slotC = hS >> (32u - LZ_LOG_C);
        __syncthreads();
        LZ_PHASE(P, 0);    // load + hash + probe
        // ---- P2: insert (most recent position wins; first-in-chunk wins for the chunk table)
        if (canHash) {
            atomicMax(&tabL[hL >> (32u - LZ_LOG_L)], (p << LZ_TAG_BITS) | tagL);
            atomicMax(&tabS[hS >> (32u - LZ_LOG_S)], (p << LZ_TAG_BITS) | tagS);
            atomicMin(&tabC[slotC], (gen << 24) | (t << 14) | tagC);
        }
        __syncthreads();
        LZ_PHASE(P, 1);    // insert
        // ---- P3/P4: near probe + verification
        uint32_t bestLen = 0, bestOff = 0;
        if (canHash) {
            const uint32_t maxLen = (n - p) < GC_MATCH_CAP ? (n - p) : GC_MATCH_CAP;
            uint32_t cand[3]; int nc = 0;
            if (eL != 0 && (eL & ((1u << LZ_TAG_BITS) - 1u)) == tagL) cand[nc++] = eL >> LZ_TAG_BITS;
            if (eS != 0 && (eS & ((1u << LZ_TAG_BITS) - 1u)) == tagS) { uint32_t c = eS >> LZ_TAG_BITS; if (nc == 0 || cand[0] != c) cand[nc++] = c; }
            {
                uint32_t eC = tabC[slotC];
                if ((eC >> 24) == gen && (eC & 0x3FFFu) == tagC) {
                    uint32_t tc = (eC >> 14) & 0x3FFu;
                    if (tc < t) { uint32_t c = cbase + tc; bool dup = false; for (int i = 0; i < nc; i++) dup |= cand[i] == c; if (!dup) cand[nc++] = c; }
                }
            }
            if constexpr (DICT) {
                const uint32_t dtL = (hL >> (32u - LZ_LOG_DICT - LZ_TAG_BITS)) & ((1u << LZ_TAG_BITS) - 1u), dtS = (hS >> (32u - LZ_LOG_DICT - LZ_TAG_BITS)) & ((1u << LZ_TAG_BITS) - 1u);
                uint32_t q0 = 0, q1 = 0;                      // dictionary position + 1 of the long-hash and the short-hash candidate (0: none)
                if (dL != 0u && (dL & ((1u << LZ_TAG_BITS) - 1u)) == dtL) q0 = dL >> LZ_TAG_BITS;
                if (dS != 0u && (dS & ((1u << LZ_TAG_BITS) - 1u)) == dtS && (dS >> LZ_TAG_BITS) != q0) q1 = dS >> LZ_TAG_BITS;
                lz_verify_dict(src + base, (uint32_t)(end - base), p, me, cand, nc, D, q0, q1, maxLen, bestLen, bestOff);
            } else
            lz_verify(src + base, p, me, cand, nc, maxLen, bestLen, bestOff);
        }
        // prefetch the next chunk's own bytes; the latency hides under the parse below
        if constexpr (DICT) { if (p + LZ_T < n) own = lz_ld16_end(src, base + p + LZ_T, end); }
        else if (base + p + LZ_T + GC_MATCH_CAP + 16u <= end) own = lz_ld16(src, base + p + LZ_T);
        S.sM[t] = (bestOff << 8) | bestLen;
        __syncthreads();
        if constexpr (DICT) {
            // ---- P4b: continuation of capped matches.  A match longer than GC_MATCH_CAP is a chain of capped records at one offset, and the parse hops from
            //      one to the next -- but each record has to find that offset through the hash tables on its own, and a dictionary table keeps one position per
            //      slot.  So every position also tries the offsets of the capped records GC_MATCH_CAP, 2 * GC_MATCH_CAP, ... in front of it (the records of this
            //      step as P4 left them, then the one the previous step ended with in this residue class): the first two distinct ones.  A record is valid by
            //      its own compare, whatever the chain; an offset from the chain wins when it matches at least as far as the position's own candidate.
            uint32_t h0 = 0, h1 = 0;
            for (uint32_t a = t; a >= GC_MATCH_CAP && !h1; ) {
                a -= GC_MATCH_CAP;
                const uint32_t r = S.sM[a];
                if ((r & 0xFFu) == GC_MATCH_CAP) { if (!h0) h0 = r >> 8; else if ((r >> 8) != h0) h1 = r >> 8; }
            }
            if (!h1) {
                const uint32_t r = D.sTail[t & (GC_MATCH_CAP - 1u)];
                if ((r & 0xFFu) == GC_MATCH_CAP) { if (!h0) h0 = r >> 8; else if ((r >> 8) != h0) h1 = r >> 8; }
            }
            uint32_t nLen = bestLen, nOff = bestOff;
            if (inBlock && n - p >= GC_MIN_MATCH) {
                const uint32_t maxLen = (n - p) < GC_MATCH_CAP ? (n - p) : GC_MATCH_CAP;
                if (h0 && h0 != nOff) { const uint32_t len = lz_len_at(src + base, (uint32_t)(end - base), p, me, h0, D, maxLen); if (len >= GC_MIN_MATCH && len >= nLen) { nLen = len; nOff = h0; } }
                if (h1 && h1 != nOff) { const uint32_t len = lz_len_at(src + base, (uint32_t)(end - base), p, me, h1, D, maxLen); if (len >= GC_MIN_MATCH && len > nLen) { nLen = len; nOff = h1; } }
            }
            __syncthreads();                                  // (every position has read the records in front of it)
            bestLen = nLen; bestOff = nOff;
            S.sM[t] = (bestOff << 8) | bestLen;
            if (t >= LZ_T - GC_MATCH_CAP) D.sTail[t & (GC_MATCH_CAP - 1u)] = (bestOff << 8) | bestLen;
            __syncthreads();
        }
        LZ_PHASE(P, 2);    // verify
        lz_parse_emit(S, P, cbase, inBlock, bestLen, bestOff, src + base, mySeq, myLit, totalSeq, totalLit);
    }
    if (prof && t == 0) for (int i = 0; i < GC_LZ_PHASES; i++) atomicAdd(&prof[i], P.pc[i]);
    if (t == 0) { GcBlockMeta m; m.nSeqRaw = totalSeq; m.nLit = totalLit; *myMeta = m; }
}

#define LZ_BLOCK_LDS \
    __shared__ uint32_t tabL[1u << LZ_LOG_L]; \
    __shared__ uint32_t tabS[1u << LZ_LOG_S]; \
    __shared__ uint32_t tabC[1u << LZ_LOG_C]; \
    __shared__ LzParseLds S

// K1: block b = bytes [b * 128 KiB, ...) of one stream of srcSize bytes
extern "C" __global__ void __launch_bounds__(LZ_T)
gc_zstd_lz_kernel(const uint8_t* __restrict__ src, uint64_t srcSize, GcSeqRaw* __restrict__ seqRaw,
                  uint8_t* __restrict__ lit, GcBlockMeta* __restrict__ meta,
                  unsigned long long* __restrict__ prof /* optional: per-phase cycle sums (thread 0 of every block) */)
{
    LZ_BLOCK_LDS;
    const uint32_t b = blockIdx.x;
    const uint64_t base = (uint64_t)b * GC_ZSTD_BLOCK_MAX;
    const uint32_t n = (uint32_t)((srcSize - base) < GC_ZSTD_BLOCK_MAX ? (srcSize - base) : GC_ZSTD_BLOCK_MAX);
    lz_block<false>(src, base, n, srcSize, seqRaw + (uint64_t)b * GC_MAX_SEQ_PER_BLOCK, lit + (uint64_t)b * GC_ZSTD_BLOCK_MAX, meta + b, prof, tabL, tabS, tabC, S);
}

// K1b: workgroup b takes item b of a batch (gc_zstd_batch.h): bytes [src_off, src_off + src_size) of src, at most one block, at any alignment.  The item's end
// stands where K1 has the stream's end, so nothing outside the item is read and the matches are those of a stream call on the item alone.
extern "C" __global__ void __launch_bounds__(LZ_T)
gc_zstd_lz_batch_kernel(const uint8_t* __restrict__ src, const gc_batch_item* __restrict__ items, GcSeqRaw* __restrict__ seqRaw,
                        uint8_t* __restrict__ lit, GcBlockMeta* __restrict__ meta)
{
    LZ_BLOCK_LDS;
    const uint32_t b = blockIdx.x;
    const gc_batch_item it = items[b];
    lz_block<false>(src, it.src_off, it.src_size, it.src_off + it.src_size, seqRaw + (uint64_t)b * GC_MAX_SEQ_PER_BLOCK, lit + (uint64_t)b * GC_ZSTD_BLOCK_MAX, meta + b, nullptr,
             tabL, tabS, tabC, S);
}

// K1b with a dictionary: as K1b, the dictionary (bytes and digest of the context, gc_zstd_set_dictionary) as history in front of every item
extern "C" __global__ void __launch_bounds__(LZ_T)
gc_zstd_lz_batch_dict_kernel(const uint8_t* __restrict__ src, const gc_batch_item* __restrict__ items, GcSeqRaw* __restrict__ seqRaw,
                             uint8_t* __restrict__ lit, GcBlockMeta* __restrict__ meta,
                             const uint8_t* __restrict__ dict, uint32_t dictSize, const uint32_t* __restrict__ dTabL, const uint32_t* __restrict__ dTabS)
{
    LZ_BLOCK_LDS;
    const uint32_t b = blockIdx.x;
    const gc_batch_item it = items[b];
    __shared__ uint32_t sTail[GC_MATCH_CAP];
    LzDict D; D.bytes = dict; D.tabL = dTabL; D.tabS = dTabS; D.size = dictSize; D.sTail = sTail;
    lz_block<true>(src, it.src_off, it.src_size, it.src_off + it.src_size, seqRaw + (uint64_t)b * GC_MAX_SEQ_PER_BLOCK, lit + (uint64_t)b * GC_ZSTD_BLOCK_MAX, meta + b, nullptr,
                   tabL, tabS, tabC, S, D);
}

// The dictionary's digest, once per gc_zstd_set_dictionary: every position with 8 readable bytes is hashed with K1's two functions into two tables of
// 2^LZ_LOG_DICT entries; atomicMax = "most recent position wins", as K1's P2, so the tables do not depend on the order the lanes arrive in.
// The tables start zeroed.  One thread per position.
extern "C" __global__ void __launch_bounds__(256)
gc_zstd_dict_digest_kernel(const uint8_t* __restrict__ dict, uint32_t dictSize, uint32_t* __restrict__ dTabL, uint32_t* __restrict__ dTabS)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p + 8u > dictSize) return;
    const LzW16 w = lz_ld16(dict, p);                        // (the buffer is padded: gc_zstd_set_dictionary)
    const uint32_t lo = (uint32_t)w.a, hi = (uint32_t)(w.a >> 32);
    const uint32_t hL = lz_hash_long(lo, hi), hS = lz_hash_short(lo, hi);
    const uint32_t tagL = (hL >> (32u - LZ_LOG_DICT - LZ_TAG_BITS)) & ((1u << LZ_TAG_BITS) - 1u);
    const uint32_t tagS = (hS >> (32u - LZ_LOG_DICT - LZ_TAG_BITS)) & ((1u << LZ_TAG_BITS) - 1u);
    atomicMax(&dTabL[hL >> (32u - LZ_LOG_DICT)], ((p + 1u) << LZ_TAG_BITS) | tagL);
    atomicMax(&dTabS[hS >> (32u - LZ_LOG_DICT)], ((p + 1u) << LZ_TAG_BITS) | tagS);
}
