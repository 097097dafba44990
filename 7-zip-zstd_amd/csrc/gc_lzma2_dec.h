// gc_lzma2_dec.h -- LZMA2 decoder (7-Zip method id 0x21): what NCompress::NLzma2::CDecoder (CPP/7zip/Compress/Lzma2Decoder.cpp) runs through
// Lzma2Dec_DecodeToDic (C/Lzma2Dec.c: chunk walk, control bytes, props rules) and LzmaDec_DecodeReal (C/LzmaDec.c: symbol grammar, state machine, range decoder).
// Included once, from gc_lzma2_frame.hip (kernels and host side), so that the product build and the emulator build take it through a unit they already list.
//
// A UNIT is a run of chunks that starts with a dictionary reset (control 0x01 or >= 0xE0) and ends in front of the next one or of the end marker.  Units are independent
// of each other -- the split C/Lzma2DecMt.c makes for its threads -- and nothing inside a unit is: every bit goes through the adaptive range decoder, the literal coder
// is chosen by the byte in front, a matched literal is coded against the byte at the last distance.  So: ONE WAVE PER UNIT, dealt through a ticket (largest unit first),
// the grid bounded by what the device holds at once.  No wave waits for another wave: no flag, no spin, no dependency between units.
//
// Inside the wave the decoder's state (range, code, state, four distances, positions, chunk bookkeeping) is the same in every lane and written as plain wave-uniform
// code (scalar registers).  What is wide is done by the wave together: the bytes of a match (lane i writes byte i; a copy that overlaps itself reads `i mod distance`),
// stored chunks, the reset of the probability table, the hand-over of the output to HBM.
//   input    16 bytes per lane and load: the KB at the read position lies in four vector registers of the wave (`win`), the KB behind it is in flight (`pend`);
//            eight bytes at a time move to a scalar accumulator through v_readlane.  Chunk headers are read through the same reader (a unit is contiguous).
//   probs    11-bit counters in 16-bit LDS words, LzmaDec.c's 1 984 + (0x300 << (lc + lp)); lane 0 stores the update.
//   output   the last RING bytes live in an LDS ring (previous byte, match byte, near matches); the ring is handed to HBM in whole 64-byte lines, 16 bytes per lane,
//            when it is nearly full (a far match whose source has not been handed over yet, a stored chunk and the unit's end hand over what there is);
//            far matches read HBM behind what has been handed over.
// Instances (LDS per wave -> waves per CU of 160 KiB; one wave per workgroup):
//   a   lc + lp <= 3   probs 16 256 B + ring 16 384 B = 32 640 B   -> 5 waves per CU   (the usual lc 3 / lp 0: the larger ring keeps more matches in LDS)
//   b   lc + lp <= 4   probs 28 544 B + ring  8 192 B = 36 736 B   -> 4 waves per CU   (one per SIMD)
// A call that holds units of both kinds launches a, then b, on the context's one stream: the two groups run one after the other (b starts when a's last unit is out),
// not side by side.  Streams mix them rarely (one encoder, one setting), so the idle tail of a is accepted rather than paid for with a second stream.
// The compiler holds the wave-uniform state in 106 scalar registers and parks 8 more values in lanes of a vector register (SGPR spill to VGPR: no scratch memory).
// Props may change inside a unit (this engine's encoder chooses lc / lp per model segment), so the scan reports a unit's LARGEST lc + lp and the host sends it to the
// instance that holds it; a unit that meets a larger one than its instance holds (wrong flags) ends with L2D_LIMIT instead of writing outside the table.
// Bounds: a symbol yields at least one byte and the chunk's unpacked size caps the bytes; reads stop at the chunk's packed size and never leave the unit's source range;
// writes stop at the unit's dst_size.
#pragma once
#include "gpucodec.h"
#include "gc_common.h"
#include "gc_device.h"
#ifdef HIPEMU
#include "hip_runtime_stub.h"
#else
#include <hip/hip_runtime.h>
#ifndef GC_LAUNCH
#define GC_LAUNCH(kernel, grid, block, stream, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__)
#endif
#endif
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "gc_lzma2_dec_work.h"

// status of one unit
#define L2D_OK          0u
#define L2D_CORRUPT     1u
#define L2D_DST_SMALL   2u
#define L2D_LIMIT       3u            // a props byte with a larger lc + lp than the kernel instance holds

#define L2D_MAX_UNITS   (1u << 20)
#define L2D_MAX_BYTES   0xFFFF0000u   // a unit's source and content sizes fit 32-bit positions with room for the reader's look-ahead

struct GcL2dUnit { uint64_t srcOff, dstOff; uint32_t srcSize, dstSize, nChunks, pad; };
struct GcL2dResult { uint32_t status, produced; };

// the probability table (C/LzmaDec.c's counters; offsets in 16-bit words)
#define L2D_IS_MATCH      0u          // [12 states][16 position states]
#define L2D_IS_REP        192u        // [12]
#define L2D_IS_REP_G0     204u
#define L2D_IS_REP_G1     216u
#define L2D_IS_REP_G2     228u
#define L2D_IS_REP0_LONG  240u        // [12][16]
#define L2D_LEN           432u        // choice, choice2, low[16][8], mid[16][8], high[256]
#define L2D_REP_LEN       946u
#define L2D_LEN_LOW       2u
#define L2D_LEN_MID       130u
#define L2D_LEN_HIGH      258u
#define L2D_POS_SLOT      1460u       // [4 length states][64]
#define L2D_SPEC_POS      1716u       // [128]
#define L2D_ALIGN         1844u       // [16]
#define L2D_LIT           1984u       // [0x300 << (lc + lp)]

struct L2dQuad { uint32_t x, y, z, w; };
// Byte reader over the unit's source; identical in every lane except win / pend (lane l holds the 16 bytes at winBase + 16 l).  Positions are "window space": relative to
// `p`, the unit's start rounded down to 16 bytes (inside the buffer), so that every load is a whole aligned quad.
struct L2dIn {
    const uint8_t* p;
    uint32_t w, lim, end;             // the next byte; where reading stops now (the chunk's packed end / the unit's end); the unit's end
    uint64_t acc; uint32_t accN;      // accN bytes at w, w + 1, ...
    uint32_t winBase;                 // win = [winBase, winBase + 1024), pend = the KB behind it
    L2dQuad win, pend;
    uint32_t over;                    // a byte behind `lim` was asked for
};
__device__ __forceinline__ L2dQuad l2d_window(const L2dIn& in, uint32_t base, uint32_t lane)
{
    L2dQuad q; q.x = q.y = q.z = q.w = 0u;
    const uint32_t o = base + 16u * lane;
    if (o + 16u <= in.end) __builtin_memcpy(&q, in.p + o, 16);
    else if (o < in.end) {                                        // the unit's last bytes: nothing behind them is touched
        uint32_t v[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) if (o + k < in.end) v[k >> 2] |= (uint32_t)in.p[o + k] << (8u * (k & 3u));
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    }
    return q;
}
__device__ __forceinline__ void l2d_take8(L2dIn& in, uint32_t rel)      // rel = w - winBase, a multiple of 8 below 1024
{
    const uint32_t l = rel >> 4;
    uint32_t lo, hi;
    if (rel & 8u) { lo = gc_readlane(in.win.z, l); hi = gc_readlane(in.win.w, l); }
    else { lo = gc_readlane(in.win.x, l); hi = gc_readlane(in.win.y, l); }
    in.acc = (uint64_t)lo | ((uint64_t)hi << 32); in.accN = 8u;
}
__device__ __forceinline__ void l2d_prime(L2dIn& in, uint32_t w, uint32_t lane)
{
    in.w = w; in.winBase = w & ~15u;
    in.win = l2d_window(in, in.winBase, lane); in.pend = l2d_window(in, in.winBase + 1024u, lane);
    l2d_take8(in, w & 8u);
    const uint32_t drop = w & 7u;
    in.acc >>= 8u * drop; in.accN = 8u - drop;
}
__device__ __forceinline__ void l2d_refill(L2dIn& in, uint32_t lane)   // acc is empty, so w is a multiple of 8
{
    uint32_t rel = in.w - in.winBase;
    if (rel >= 1024u) { in.win = in.pend; in.winBase += 1024u; in.pend = l2d_window(in, in.winBase + 1024u, lane); rel -= 1024u; }
    l2d_take8(in, rel);
}
__device__ __forceinline__ uint32_t l2d_byte(L2dIn& in, uint32_t lane);
__device__ __forceinline__ uint32_t l2d_be(L2dIn& in, uint32_t nbytes, uint32_t lane)      // big-endian number of nbytes bytes (chunk headers, the range coder's first code)
{
    uint32_t v = 0u;
#pragma unroll 1
    for (uint32_t k = 0; k < nbytes; k++) v = (v << 8) | l2d_byte(in, lane);
    return v;
}
__device__ __forceinline__ uint32_t l2d_byte(L2dIn& in, uint32_t lane)
{
    if (in.w >= in.lim) { in.over = 1u; return 0u; }
    if (in.accN == 0u) l2d_refill(in, lane);
    const uint32_t b = (uint32_t)in.acc & 0xFFu;
    in.acc >>= 8; in.accN--; in.w++;
    return b;
}

// range decoder (LzmaDec.c NORMALIZE / GET_BIT2): range and code in scalar registers, the counter in LDS.  All lanes read the counter, lane 0 stores its update; the
// step mark between the two keeps the emulator's lanes (which run one after another) from reading a counter another lane has already updated -- two bits in a row never
// use the same counter.
struct L2dRc { uint32_t range, code; };
__device__ __forceinline__ void l2d_norm(L2dRc& rc, L2dIn& in, uint32_t lane)
{
    if (rc.range < (1u << 24)) { rc.range <<= 8; rc.code = (rc.code << 8) | l2d_byte(in, lane); }
}
__device__ __forceinline__ uint32_t l2d_bit(L2dRc& rc, L2dIn& in, uint16_t* P, uint32_t i, uint32_t lane)
{
    l2d_norm(rc, in, lane);
    const uint32_t p = gc_uniform(P[i]);
    gc_wave_step();
    const uint32_t bound = (rc.range >> 11) * p;
    if (rc.code < bound) { rc.range = bound; if (lane == 0u) P[i] = (uint16_t)(p + ((2048u - p) >> 5)); return 0u; }
    rc.range -= bound; rc.code -= bound;
    if (lane == 0u) P[i] = (uint16_t)(p - (p >> 5));
    return 1u;
}
__device__ __forceinline__ uint32_t l2d_tree(L2dRc& rc, L2dIn& in, uint16_t* P, uint32_t base, uint32_t nbits, uint32_t lane)
{
    uint32_t m = 1u;
#pragma unroll 1
    for (uint32_t k = 0; k < nbits; k++) m = (m << 1) | l2d_bit(rc, in, P, base + m, lane);
    return m - (1u << nbits);
}
__device__ __forceinline__ uint32_t l2d_tree_rev(L2dRc& rc, L2dIn& in, uint16_t* P, uint32_t base, uint32_t nbits, uint32_t lane)
{
    uint32_t m = 1u, v = 0u;
#pragma unroll 1
    for (uint32_t k = 0; k < nbits; k++) { const uint32_t b = l2d_bit(rc, in, P, base + m, lane); m = (m << 1) | b; v |= b << k; }
    return v;
}
__device__ __forceinline__ uint32_t l2d_len(L2dRc& rc, L2dIn& in, uint16_t* P, uint32_t base, uint32_t posState, uint32_t lane)
{
    // (one tree walk whichever of low / mid / high it is: every inlined copy of the bit decoder is instruction-cache footprint)
    uint32_t tree = base + L2D_LEN_LOW + posState * 8u, nbits = 3u, add = 0u;
    if (l2d_bit(rc, in, P, base, lane)) {
        if (!l2d_bit(rc, in, P, base + 1u, lane)) { tree = base + L2D_LEN_MID + posState * 8u; add = 8u; }
        else { tree = base + L2D_LEN_HIGH; nbits = 8u; add = 16u; }
    }
    return add + l2d_tree(rc, in, P, tree, nbits, lane);
}

// Output [from, upto) from the ring to HBM: 16 bytes per lane where the address is aligned (the ring's index carries the address's low bits, `skew`), single bytes at a
// ragged head or tail.
template <uint32_t RING>
__device__ __forceinline__ void l2d_flush(const uint8_t* ring, uint8_t* __restrict__ out, uint32_t skew, uint32_t from, uint32_t upto, uint32_t lane)
{
    constexpr uint32_t RMASK = RING - 1u;
    gc_wave_sync();
    uint32_t a = from;
    const uint32_t head = (16u - ((a + skew) & 15u)) & 15u, h = head < upto - a ? head : upto - a;
    if (lane < h) out[a + lane] = ring[(a + lane + skew) & RMASK];
    a += h;
    const uint32_t n16 = (upto - a) >> 4;
    struct alignas(16) V16 { uint64_t x, y; };
    for (uint32_t k = lane; k < n16; k += 64u) *(V16*)(out + a + 16u * k) = *(const V16*)(ring + ((a + 16u * k + skew) & RMASK));
    a += n16 << 4;
    if (lane < upto - a) out[a + lane] = ring[(a + lane + skew) & RMASK];
    gc_wave_step();
}

// ------------------------------------------------------------------------------------------------ one wave per unit
template <uint32_t LCLP, uint32_t RING>
__device__ __forceinline__ void l2d_kernel_body(const uint8_t* __restrict__ src, const GcL2dUnit* __restrict__ units, const uint32_t* __restrict__ order, uint32_t nUnits,
                                                uint32_t* __restrict__ ticket, uint8_t* __restrict__ dst, GcL2dResult* __restrict__ result, uint32_t dictSize)
{
    constexpr uint32_t NPROB = L2D_LIT + (0x300u << LCLP);
    constexpr uint32_t RMASK = RING - 1u;
    static_assert(RING >= 4096u && (RING & (RING - 1u)) == 0u, "the ring holds the longest match beside what it has not handed over");
    __shared__ __attribute__((aligned(16))) uint16_t sProb[NPROB];
    __shared__ __attribute__((aligned(16))) uint8_t sRing[RING];
    const uint32_t lane = threadIdx.x;
    uint16_t* const P = sProb;
    for (;;) {
        uint32_t t = 0u;
        if (lane == 0u) t = atomicAdd(ticket, 1u);
        t = gc_uniform(__shfl(t, 0));
        if (t >= nUnits) break;
        const uint32_t u = gc_uniform(order[t]);
        const GcL2dUnit un = units[u];
        const uint32_t dstSize = gc_uniform(un.dstSize), nChunks = gc_uniform(un.nChunks);
        uint8_t* const out = dst + un.dstOff;
        const uint32_t skew = gc_uniform((uint32_t)((uintptr_t)out & 63u));
        const uint32_t skewIn = gc_uniform((uint32_t)(un.srcOff & 15u));
        L2dIn in; in.p = src + (un.srcOff - skewIn); in.end = skewIn + gc_uniform(un.srcSize); in.lim = in.end; in.over = 0u;
        l2d_prime(in, skewIn, lane);
        L2dRc rc; rc.range = 0u; rc.code = 0u;
        uint32_t status = L2D_OK, pos = 0u, flushed = 0u;          // output [flushed, pos) is in the ring only
        bool unfenced = false;                                    // the wave has stored to HBM since it last waited for its stores
        uint32_t lc = 0u, lpMask = 0u, pbMask = 0u, state = 0u, rep0 = 0u, rep1 = 0u, rep2 = 0u, rep3 = 0u, prev = 0u;
        bool hasProps = false;
        for (uint32_t c = 0; c < nChunks && status == L2D_OK; c++) {
            in.lim = in.end;
            const uint32_t ctl = l2d_byte(in, lane);
            const bool dicReset = ctl == 1u || ctl >= 0xE0u;
            if (in.over || ctl == 0u || (ctl >= 3u && ctl < 0x80u) || dicReset != (c == 0u)) { status = L2D_CORRUPT; break; }
            if (ctl < 0x80u) {
                // ---- stored chunk: source -> HBM and the ring's tail; the coder's state stays (LzmaDec_InitDicAndState(initDic, False))
                const uint32_t n = l2d_be(in, 2u, lane) + 1u;
                if (in.over || n > in.end - in.w) { status = L2D_CORRUPT; break; }
                if (n > dstSize - pos) { status = L2D_DST_SMALL; break; }
                l2d_flush<RING>(sRing, out, skew, flushed, pos, lane);
                const uint8_t* const s = in.p + in.w;
                for (uint32_t i = lane; i < n; i += 64u) { const uint8_t v = s[i]; out[pos + i] = v; if (i + RING >= n) sRing[(pos + i + skew) & RMASK] = v; }
                pos += n; flushed = pos; unfenced = true;
                gc_wave_sync();
                prev = gc_uniform(sRing[(pos - 1u + skew) & RMASK]);
                l2d_prime(in, in.w + n, lane);
                continue;
            }
            // ---- LZMA chunk
            const uint32_t sizes = l2d_be(in, 4u, lane);
            const uint32_t usize = (((ctl & 0x1Fu) << 16) | (sizes >> 16)) + 1u, csize = (sizes & 0xFFFFu) + 1u;
            const uint32_t reset = (ctl >> 5) & 3u;
            if (reset >= 2u) {
                uint32_t pr = l2d_byte(in, lane);
                if (in.over || pr >= 225u) { status = L2D_CORRUPT; break; }
                lc = pr % 9u; pr /= 9u;
                const uint32_t lp = pr % 5u, pb = pr / 5u;
                if (lc + lp > 4u) { status = L2D_CORRUPT; break; }
                if (lc + lp > LCLP) { status = L2D_LIMIT; break; }
                lpMask = (1u << lp) - 1u; pbMask = (1u << pb) - 1u; hasProps = true;
            } else if (!hasProps) { status = L2D_CORRUPT; break; }     // (Lzma2Dec_UpdateState: needInitLevel)
            if (in.over || csize > in.end - in.w) { status = L2D_CORRUPT; break; }
            if (usize > dstSize - pos) { status = L2D_DST_SMALL; break; }
            if (reset >= 1u) {
                const uint32_t words = (L2D_LIT + (0x300u << (lc + __popc(lpMask)))) >> 1;
                gc_wave_sync();
                for (uint32_t i = lane; i < words; i += 64u) ((uint32_t*)sProb)[i] = 0x04000400u;
                gc_wave_sync();
                state = 0u; rep0 = rep1 = rep2 = rep3 = 0u;
            }
            in.lim = in.w + csize;
            if (csize < 5u || l2d_be(in, 1u, lane) != 0u) { status = L2D_CORRUPT; break; }      // the first byte of a range coder's output is 0 (LzmaDec.c)
            rc.range = 0xFFFFFFFFu; rc.code = l2d_be(in, 4u, lane);
            uint32_t left = usize;
            while (left != 0u) {
                if (pos - flushed + 273u + 64u > RING) {           // hand the whole lines over: room for the longest match
                    const uint32_t upto = ((pos + skew) & ~63u) - skew;
                    l2d_flush<RING>(sRing, out, skew, flushed, upto, lane);
                    flushed = upto; unfenced = true;
                }
                const uint32_t posState = pos & pbMask;
                if (!l2d_bit(rc, in, P, L2D_IS_MATCH + state * 16u + posState, lane)) {
                    // ---- literal
                    const uint32_t lit = L2D_LIT + 0x300u * (((pos & lpMask) << lc) + (prev >> (8u - lc)));
                    // one loop for both kinds: with offs = 0 the matched literal's walk IS the plain one (every term of the match byte is masked away)
                    uint32_t sym = 1u, mb = 0u, offs = 0u;
                    if (state >= 7u) {
                        const uint32_t q = pos - rep0 - 1u;         // (state >= 7: rep0 was checked against the position when it was set)
                        if (pos - q <= RING) mb = gc_uniform(sRing[(q + skew) & RMASK]);
                        else { if (unfenced) { gc_wave_sync_global(); unfenced = false; } mb = gc_uniform(out[q]); }
                        offs = 0x100u;
                    }
#pragma unroll 1
                    do {
                        mb <<= 1;
                        const uint32_t m = mb & offs, bit = l2d_bit(rc, in, P, lit + offs + m + sym, lane);
                        sym = (sym << 1) | bit;
                        offs &= bit ? mb : ~mb;
                    } while (sym < 0x100u);
                    prev = sym & 0xFFu;
                    if (lane == 0u) sRing[(pos + skew) & RMASK] = (uint8_t)prev;
                    pos++; left--;
                    state = state < 4u ? 0u : (state < 10u ? state - 3u : state - 6u);
                } else {
                    const bool isRep = l2d_bit(rc, in, P, L2D_IS_REP + state, lane) != 0u;
                    if (isRep) {
                        if (!l2d_bit(rc, in, P, L2D_IS_REP_G0 + state, lane)) {
                            if (!l2d_bit(rc, in, P, L2D_IS_REP0_LONG + state * 16u + posState, lane)) {
                                // ---- short rep: one byte at the last distance
                                if (rep0 >= pos || rep0 >= dictSize) { status = L2D_CORRUPT; break; }
                                const uint32_t q = pos - rep0 - 1u;
                                if (pos - q <= RING) prev = gc_uniform(sRing[(q + skew) & RMASK]);
                                else { if (unfenced) { gc_wave_sync_global(); unfenced = false; } prev = gc_uniform(out[q]); }
                                if (lane == 0u) sRing[(pos + skew) & RMASK] = (uint8_t)prev;
                                pos++; left--;
                                state = state < 7u ? 9u : 11u;
                                if (in.over) { status = L2D_CORRUPT; break; }
                                continue;
                            }
                        } else {
                            uint32_t d;
                            if (!l2d_bit(rc, in, P, L2D_IS_REP_G1 + state, lane)) d = rep1;
                            else {
                                if (!l2d_bit(rc, in, P, L2D_IS_REP_G2 + state, lane)) d = rep2;
                                else { d = rep3; rep3 = rep2; }
                                rep2 = rep1;
                            }
                            rep1 = rep0; rep0 = d;
                        }
                    }
                    uint32_t len = l2d_len(rc, in, P, isRep ? L2D_REP_LEN : L2D_LEN, posState, lane);      // (one inlined copy of the length decoder for both)
                    if (isRep) state = state < 7u ? 8u : 11u;
                    else {
                        // ---- match: distance slot, distance
                        const uint32_t slot = l2d_tree(rc, in, P, L2D_POS_SLOT + (len < 4u ? len : 3u) * 64u, 6u, lane);
                        uint32_t dist = slot;
                        if (slot >= 4u) {
                            const uint32_t nd = (slot >> 1) - 1u;
                            dist = (2u | (slot & 1u)) << nd;
                            if (slot < 14u) dist += l2d_tree_rev(rc, in, P, L2D_SPEC_POS + dist - slot, nd, lane);
                            else {
                                uint32_t v = 0u;                    // direct bits: no counters
#pragma unroll 1
                                for (uint32_t k = nd - 4u; k != 0u; k--) { l2d_norm(rc, in, lane); rc.range >>= 1; v <<= 1; if (rc.code >= rc.range) { rc.code -= rc.range; v |= 1u; } }
                                dist += v << 4;
                                dist += l2d_tree_rev(rc, in, P, L2D_ALIGN, 4u, lane);
                            }
                        }
                        rep3 = rep2; rep2 = rep1; rep1 = rep0; rep0 = dist;
                        state = state < 7u ? 7u : 10u;
                    }
                    len += 2u;
                    // (the end-of-payload marker, distance 0xFFFFFFFF, fails the first test: LZMA2 chunks do not use it)
                    if (in.over || rep0 >= pos || rep0 >= dictSize || len > left) { status = L2D_CORRUPT; break; }
                    const uint32_t d = rep0 + 1u;
                    gc_wave_sync();                               // lane 0's literals in the ring
                    if (d + len <= RING) {
                        // near: no slot this copy writes holds a byte it still reads, in whatever order the lanes run
                        for (uint32_t i = lane; i < len; i += 64u) { const uint8_t v = sRing[(pos - d + (d < len ? i % d : i) + skew) & RMASK]; sRing[(pos + i + skew) & RMASK] = v; }
                    } else {
                        // far (d > RING - 273, so the copy does not overlap itself): the source is in HBM once the ring has handed it over
                        if (pos - d + len > flushed) { l2d_flush<RING>(sRing, out, skew, flushed, pos, lane); flushed = pos; unfenced = true; }
                        if (unfenced) { gc_wave_sync_global(); unfenced = false; }
                        const uint8_t* const s = out + (pos - d);
                        for (uint32_t i = lane; i < len; i += 64u) sRing[(pos + i + skew) & RMASK] = s[i];
                    }
                    pos += len; left -= len;
                    gc_wave_sync();
                    prev = gc_uniform(sRing[(pos - 1u + skew) & RMASK]);
                }
                if (in.over) { status = L2D_CORRUPT; break; }
            }
            if (status != L2D_OK) break;
            // the chunk's bytes are out: its payload must be used up and the coder at rest (Lzma2Dec.c asks for LZMA_STATUS_MAYBE_FINISHED_WITHOUT_MARK and packSize == 0)
            l2d_norm(rc, in, lane);
            if (in.over || in.w != in.lim || rc.code != 0u) status = L2D_CORRUPT;
        }
        if (status == L2D_OK && (pos != dstSize || in.w != in.end)) status = L2D_CORRUPT;       // (the scan's numbers are exact)
        l2d_flush<RING>(sRing, out, skew, flushed, pos, lane);
        if (lane == 0u) { GcL2dResult r; r.status = status; r.produced = pos; result[u] = r; }
        gc_wave_sync();
    }
}
#define L2D_INSTANCE(NAME, LCLP, RING) \
extern "C" __global__ void __launch_bounds__(64) NAME(const uint8_t* __restrict__ src, const GcL2dUnit* __restrict__ units, const uint32_t* __restrict__ order, uint32_t nUnits, \
    uint32_t* __restrict__ ticket, uint8_t* __restrict__ dst, GcL2dResult* __restrict__ result, uint32_t dictSize) \
{ l2d_kernel_body<LCLP, RING>(src, units, order, nUnits, ticket, dst, result, dictSize); }
L2D_INSTANCE(gc_lzma2_dec_kernel_a, 3u, 16384u)      // lc + lp <= 3: five waves per CU
L2D_INSTANCE(gc_lzma2_dec_kernel_b, 4u, 8192u)       // lc + lp <= 4: four
#define L2D_WAVES_A 5u
#define L2D_WAVES_B 4u

// ------------------------------------------------------------------------------------------------ host side
// Walks the chunk headers of an LZMA2 stream (Lzma2Dec_UpdateState's rules; both sizes are in the header, so no payload is read).  units may be null (count only).
extern "C" int gc_lzma2_scan_prefix(const void* src, size_t n, gc_lzma2_unit* units, size_t maxUnits, size_t* nUnits, uint64_t* contentTotal, size_t* consumed, int* ended)
{
    if ((!src && n) || !nUnits) return GC_ERR_PARAM;
    const uint8_t* p = (const uint8_t*)src;
    size_t off = 0, k = 0, done = 0; uint64_t total = 0; int end = 0;
    bool open = false, hasProps = false;
    gc_lzma2_unit cur; memset(&cur, 0, sizeof(cur));
    for (;;) {
        if (off >= n) break;                                      // the input ends inside a unit (or in front of the first)
        const uint32_t ctl = p[off];
        const bool closes = ctl == 0u || ctl == 1u || ctl >= 0xE0u;
        if (ctl >= 3u && ctl < 0x80u) return GC_ERR_CORRUPT;
        if (!open && ctl != 0u && !closes) return GC_ERR_CORRUPT;  // the first chunk must reset the dictionary
        if (closes && open) {                                     // the unit in front is whole
            cur.src_size = off - cur.src_off;
            if (ctl == 0u) cur.flags |= 0x100u;
            if (units) { if (k >= maxUnits) return GC_ERR_PARAM; units[k] = cur; }
            k++; total += cur.dst_size; done = off; open = false;
        }
        if (ctl == 0u) { end = 1; done = off + 1u; break; }
        if (closes) { memset(&cur, 0, sizeof(cur)); cur.src_off = off; cur.dst_off = total; open = true; hasProps = false; }
        if (ctl < 0x80u) {
            if (off + 3u > n) break;
            const size_t sz = (((size_t)p[off + 1] << 8) | p[off + 2]) + 1u;
            cur.dst_size += sz; cur.n_chunks++;
            off += 3u + sz;
        } else {
            const size_t hdr = (ctl & 0x40u) ? 6u : 5u;
            if (off + hdr > n) break;
            if (ctl & 0x40u) {
                const uint32_t pr = p[off + 5];
                if (pr >= 225u) return GC_ERR_CORRUPT;
                const uint32_t lclp = pr % 9u + (pr / 9u) % 5u;
                if (lclp > 4u) return GC_ERR_CORRUPT;
                if (lclp > (cur.flags & 7u)) cur.flags = (cur.flags & ~7u) | lclp;
                hasProps = true;
            } else if (!hasProps) return GC_ERR_CORRUPT;          // (needInitLevel: no props yet in this unit)
            cur.dst_size += ((((size_t)ctl & 0x1Fu) << 16) | ((size_t)p[off + 1] << 8) | p[off + 2]) + 1u;
            cur.n_chunks++;
            off += hdr + ((((size_t)p[off + 3] << 8) | p[off + 4]) + 1u);
        }
    }
    *nUnits = k;
    if (contentTotal) *contentTotal = total;
    if (consumed) *consumed = done;
    if (ended) *ended = end;
    return GC_OK;
}

void gc_l2d_release(GcL2dWork* w)      // (the events: the buffers free themselves with the context)
{
    if (w->ev0) hipEventDestroy((hipEvent_t)w->ev0);
    if (w->ev1) hipEventDestroy((hipEvent_t)w->ev1);
    w->ev0 = w->ev1 = nullptr;
}
// d_src / d_dst: device memory; units: host memory (as the scan returned them).  Synchronous (the units' results are read back).
int gc_l2d_decode(hipStream_t st, GcL2dWork* w, const uint8_t* d_src, size_t n, const gc_lzma2_unit* units, size_t nUnits, uint8_t* d_dst, size_t dstCap, unsigned dictProp,
                  size_t* produced, char* err, size_t errCap)
{
    *produced = 0;
    w->ms = 0.0f;
    if (dictProp > 40u) return GC_ERR_PARAM;
    if (nUnits > L2D_MAX_UNITS) { if (err) snprintf(err, errCap, "%zu LZMA2 units in one call: at most %u", nUnits, L2D_MAX_UNITS); return GC_ERR_PARAM; }
    if (nUnits == 0) return GC_OK;
    const uint32_t dictSize = dictProp == 40u ? 0xFFFFFFFFu : (2u | (dictProp & 1u)) << (dictProp / 2u + 11u);      // LZMA2_DIC_SIZE_FROM_PROP
    uint64_t need = 0;
    for (size_t i = 0; i < nUnits; i++) {
        const gc_lzma2_unit& u = units[i];
        if (u.src_off > n || u.src_size > n - u.src_off) { if (err) snprintf(err, errCap, "LZMA2 unit %zu lies outside the %zu input bytes", i, n); return GC_ERR_PARAM; }
        if (u.src_size > L2D_MAX_BYTES || u.dst_size > L2D_MAX_BYTES) { if (err) snprintf(err, errCap, "LZMA2 unit %zu is larger than 4 GiB - 64 KiB", i); return GC_ERR_UNSUPPORTED; }
        if (u.dst_off > dstCap || u.dst_size > dstCap - u.dst_off) need = ~0ull;          // (no sum of the caller's numbers that could wrap)
        else if (u.dst_off + u.dst_size > need) need = u.dst_off + u.dst_size;
    }
    if (need == ~0ull) { if (err) snprintf(err, errCap, "destination too small: a unit's dst_off + dst_size lies behind the %zu bytes of capacity", dstCap); return GC_ERR_DST_SMALL; }
    if (need > dstCap) { if (err) snprintf(err, errCap, "destination too small: need %llu bytes", (unsigned long long)need); return GC_ERR_DST_SMALL; }
    // descriptors; the order: the units of instance a, then those of instance b, each largest first (the last waves to finish hold small units)
    const size_t oUnits = 0, oOrder = (nUnits * sizeof(GcL2dUnit) + 63u) & ~(size_t)63u, oRes = oOrder + ((nUnits * 4u + 63u) & ~(size_t)63u),
                 oTick = oRes + ((nUnits * sizeof(GcL2dResult) + 63u) & ~(size_t)63u), metaBytes = oTick + 64u;
    uint8_t* host = (uint8_t*)malloc(metaBytes);
    if (!host) return GC_ERR_NOMEM;
    memset(host, 0, metaBytes);
    GcL2dUnit* hu = (GcL2dUnit*)(host + oUnits); uint32_t* ho = (uint32_t*)(host + oOrder); GcL2dResult* hr = (GcL2dResult*)(host + oRes);
    uint32_t nA = 0;
    for (size_t i = 0; i < nUnits; i++) {
        hu[i].srcOff = units[i].src_off; hu[i].dstOff = units[i].dst_off; hu[i].srcSize = (uint32_t)units[i].src_size; hu[i].dstSize = (uint32_t)units[i].dst_size; hu[i].nChunks = units[i].n_chunks;
        const bool b = w->instance ? w->instance == 2u : (units[i].flags & 7u) > 3u;
        if (!b) nA++;
    }
    {
        uint32_t a = 0, b = nA;
        for (size_t i = 0; i < nUnits; i++) { const bool isB = w->instance ? w->instance == 2u : (units[i].flags & 7u) > 3u; ho[isB ? b++ : a++] = (uint32_t)i; }
        const auto larger = [hu](uint32_t i, uint32_t j) { return hu[i].srcSize != hu[j].srcSize ? hu[i].srcSize > hu[j].srcSize : i < j; };      // (the work is in the compressed bytes)
        std::sort(ho, ho + nA, larger);
        std::sort(ho + nA, ho + nUnits, larger);
    }
    int rc = gc_buf_reserve(w->meta, metaBytes, 64u);
    if (rc == GC_OK && !w->ev0 && (hipEventCreate((hipEvent_t*)&w->ev0) != hipSuccess || hipEventCreate((hipEvent_t*)&w->ev1) != hipSuccess)) rc = GC_ERR_HIP;
    if (rc == GC_OK && hipMemcpyAsync(w->meta, host, metaBytes, hipMemcpyHostToDevice, st) != hipSuccess) rc = GC_ERR_HIP;
    if (rc == GC_OK) {
        const GcL2dUnit* du = (const GcL2dUnit*)(w->meta + oUnits); const uint32_t* dord = (const uint32_t*)(w->meta + oOrder); GcL2dResult* dr = (GcL2dResult*)(w->meta + oRes);
        uint32_t* tick = (uint32_t*)(w->meta + oTick);
        const uint32_t nCU = w->nCU ? w->nCU : 256u, nB = (uint32_t)nUnits - nA;
        hipEventRecord((hipEvent_t)w->ev0, st);
        if (nA) {
            const uint32_t grid = nA < L2D_WAVES_A * nCU ? nA : L2D_WAVES_A * nCU;
            GC_LAUNCH(gc_lzma2_dec_kernel_a, grid, 64, st, d_src, du, dord, nA, tick, d_dst, dr, dictSize);
            if (hipGetLastError() != hipSuccess) rc = GC_ERR_HIP;
        }
        if (nB && rc == GC_OK) {
            const uint32_t grid = nB < L2D_WAVES_B * nCU ? nB : L2D_WAVES_B * nCU;
            GC_LAUNCH(gc_lzma2_dec_kernel_b, grid, 64, st, d_src, du, dord + nA, nB, tick + 1, d_dst, dr, dictSize);
            if (hipGetLastError() != hipSuccess) rc = GC_ERR_HIP;
        }
        hipEventRecord((hipEvent_t)w->ev1, st);
        if (rc != GC_OK) { hipStreamSynchronize(st); if (err) snprintf(err, errCap, "the LZMA2 decode kernel could not be launched"); }
        else if (hipMemcpyAsync(hr, w->meta + oRes, nUnits * sizeof(GcL2dResult), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = GC_ERR_HIP;
        if (rc == GC_OK) hipEventElapsedTime(&w->ms, (hipEvent_t)w->ev0, (hipEvent_t)w->ev1);
    }
    if (rc == GC_OK) {
        uint64_t total = 0;
        for (size_t i = 0; i < nUnits && rc == GC_OK; i++) {
            if (hr[i].status == L2D_OK) { total += hr[i].produced; continue; }
            if (hr[i].status == L2D_DST_SMALL) { rc = GC_ERR_DST_SMALL; if (err) snprintf(err, errCap, "LZMA2 unit %zu holds more than its dst_size", i); }
            else if (hr[i].status == L2D_LIMIT) { rc = GC_ERR_PARAM; if (err) snprintf(err, errCap, "LZMA2 unit %zu uses lc + lp = 4 and its flags do not say so", i); }
            else { rc = GC_ERR_CORRUPT; if (err) snprintf(err, errCap, "damaged LZMA2 stream (unit %zu, after %u of %llu bytes)", i, (unsigned)hr[i].produced, (unsigned long long)units[i].dst_size); }
        }
        if (rc == GC_OK) *produced = (size_t)total;
    }
    free(host);
    return rc;
}
