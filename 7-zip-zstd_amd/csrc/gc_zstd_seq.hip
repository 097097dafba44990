// gc_zstd_seq.hip -- K3: the sequences section of every zstd block, as FOUR kernels of different shape.
//
// Replaces ZSTD_seqToCodes (C/zstd/zstd_compress.c:2693), ZSTD_updateRep (zstd_compress_internal.h:818),
// ZSTD_buildSequencesStatistics (zstd_compress.c:2763: histograms, ZSTD_selectEncodingType, ZSTD_buildCTable ->
// FSE_normalizeCount / FSE_writeNCount / FSE_buildCTable_wksp) and ZSTD_encodeSequences_body
// (zstd_compress_sequences.c:291-383).
//
//   K3a codes   workgroup of 256 per block, parallel over sequences, SEQ_R raw records per thread and round:
//                 merge    chains of capped matches (same offset, litLength 0) collapse into one sequence
//                 repcode  repeat-offset history as a scan: rep1 = previous offset, rep2 = the offset before the current run
//                          of equal offsets.  Only codes whose meaning depends on (rep1, rep2) are emitted, so the decoder's
//                          third history slot never matters and the whole assignment is order-independent
//                 codes    LL/ML/OF code + extra bits, three histograms
//   K3b tables  ONE WAVE per (block, table): mode (predefined / RLE / FSE), normalisation, NCount header, CTable -- serial work of one lane
//   K3c chains  ONE WAVE per (block, table) walks the table's FSE state backwards over all sequences: 64 segments at once, each lane
//               finding its start state by running a few symbols ahead of its segment (FSE states forget their origin), checked and
//               repaired against the predecessor's final state, so the result is exactly the serial walk
//   K3d pack    workgroup of 256 per block, SEQ_R sequences per thread and round: per-sequence bit counts -> prefix sums -> fields OR-ed into an LDS tile -> bytes stream out
//
// Why four: as one kernel (rounds 1-2) a block held 8 waves and 53 KB of LDS for the whole time while its serial middle (tables: three
// lanes, chains: three waves; 70 % of the block's time) ran -- three blocks per CU, a machine mostly waiting.  Apart, the serial stages are
// one-wave workgroups with 3-7 KB of LDS, a few thousand of them in flight, and the parallel stages are small workgroups that come and go.
//
// Bit order is normative (zstd_compress_sequences.c:311-376): last sequence first; per sequence OF-state,
// ML-state, LL-state, LL extra, ML extra, OF extra; then final states ML, OF, LL and a closing 1 bit.
#include "gc_common.h"
#include "gc_device.h"
#include "gc_fse.h"
#include "gpucodec.h"      // gc_batch_item
#include <type_traits>
#ifdef HIPEMU
#include <stdio.h>
#include <stdlib.h>
#endif

#define SEQ_T GC_SEQ_T
#ifndef SEQ_R
#define SEQ_R 4u             // K3a / K3d: sequences per thread and round (2 or 4; profiles/seq_rounds.md has both)
#endif
#define SEQ_N (SEQ_T * SEQ_R)                            // ... per workgroup and round
#define SEQ_TILE_WORDS ((SEQ_N * 80u) / 32u + 8u)
#define SEQ_CHAIN_TILE GC_SEQ_CHAIN_TILE   // sequences per state-chain tile
#define SEQ_CHAIN_SEG  64u     // sequences per lane and tile
#define SEQ_TC(u) ((u) + ((u) >> 6))                     // index of tile element u in tCode: row stride 65 bytes (a lane walks ITS segment, i.e.
                                                         // the lanes of a wave touch elements 64 apart: unpadded they would share two LDS banks)
#ifndef SEQ_WARM_SEGS
#define SEQ_WARM_SEGS  4u      // a lane looks this many segments back for a point where all state walks meet
#endif
#define SEQ_CHK        8u      // the walk keeps its state at every 8th symbol of a segment: where a repair walk can tell that it has rejoined

__constant__ uint8_t kLLCode[64] = { 0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,16,17,17,18,18,19,19,20,20,20,20,21,21,21,21,
                                     22,22,22,22,22,22,22,22,23,23,23,23,23,23,23,23,24,24,24,24,24,24,24,24,24,24,24,24,24,24,24,24 };
__constant__ uint8_t kMLCode[128] = { 0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,
                                      32,32,33,33,34,34,35,35,36,36,36,36,37,37,37,37,38,38,38,38,38,38,38,38,39,39,39,39,39,39,39,39,
                                      40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,41,41,41,41,41,41,41,41,41,41,41,41,41,41,41,41,
                                      42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42 };
__constant__ uint8_t kLLBits[36] = { 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,6,7,8,9,10,11,12,13,14,15,16 };
__constant__ uint8_t kMLBits[53] = { 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,4,5,7,8,9,10,11,12,13,14,15,16 };
__constant__ int16_t kLLDefNorm[36] = { 4,3,2,2,2,2,2,2,2,2,2,2,2,1,1,1,2,2,2,2,2,2,2,2,2,3,2,1,1,1,1,1,-1,-1,-1,-1 };
__constant__ int16_t kMLDefNorm[53] = { 1,4,3,2,2,2,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1,-1,-1 };
__constant__ int16_t kOFDefNorm[29] = { 1,1,1,1,1,1,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1 };


struct SeqTab {              // one FSE table in LDS (K3b builds it)
    uint16_t state[512];
    GcFseSym tt[64];
    int16_t  norm[64];
    uint32_t count[64];
    uint8_t  spread[512];
    uint16_t cumul[66];
    uint8_t  desc[96];       // table description bytes for the section header
    uint32_t descSize, mode, tableLog, maxSym, finalState;
    uint32_t tabMaxSym;      // last symbol described by norm[] (predefined: whole default table)
};

// Block-wide scans of K3a / K3d (SEQ_T threads), one barrier each: the waves' totals go through sWave[par], and the caller flips `par` from call to call -- a wave
// that writes its total of call k + 2 has passed the barrier of call k + 1, which no wave reaches before it has read the totals of call k.
// exclusive sum
__device__ __forceinline__ uint32_t seq_excl_scan(uint32_t v, uint32_t (*sWave)[SEQ_T / 64u], uint32_t& par, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = gc_wave_incl_sum_dpp(v);
    uint32_t* const W = sWave[par]; par ^= 1u;
    if (lane == 63u) W[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < SEQ_T / 64u; w++) { uint32_t c = W[w]; if (w < wave) before += c; all += c; }
    *total = all;
    return before + incl - v;
}
// EXCLUSIVE max of 64-bit keys (0 in front of thread 0)
__device__ __forceinline__ uint64_t seq_excl_maxscan64(uint64_t v, uint64_t (*sWave64)[SEQ_T / 64u], uint32_t& par, uint64_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t incl = gc_wave_incl_max64_dpp(v);
    uint64_t* const W = sWave64[par]; par ^= 1u;
    if (lane == 63u) W[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (uint32_t w = 0; w < SEQ_T / 64u; w++) { const uint64_t c = W[w]; if (w < wave && c > before) before = c; if (c > all) all = c; }
    *total = all;
    const uint64_t left = ((uint64_t)gc_wave_shr1((uint32_t)(incl >> 32), 0u) << 32) | gc_wave_shr1((uint32_t)incl, 0u);      // the lane in front, 0 for lane 0
    return before > left ? before : left;
}

__device__ __forceinline__ void seq_or_bits(uint32_t* buf, uint32_t bitoff, uint64_t v, uint32_t nbits)
{
    if (nbits == 0) return;
    uint32_t word = bitoff >> 5, sh = bitoff & 31u;
    uint32_t w0 = (uint32_t)(v << sh);
    uint64_t rest = sh ? (v >> (32u - sh)) : (v >> 32);
    if (w0) atomicOr(&buf[word], w0);
    if ((uint32_t)rest) atomicOr(&buf[word + 1], (uint32_t)rest);
    if ((uint32_t)(rest >> 32)) atomicOr(&buf[word + 2], (uint32_t)(rest >> 32));
}

// Build one table (single lane).  which: 0 LL, 1 OF, 2 ML.
__device__ inline void seq_build_table(SeqTab& T, int which, uint32_t nbSeq)
{
    const uint32_t maxLog = which == 1 ? 8u : 9u, defLog = which == 1 ? 5u : 6u;
    const int16_t* defNorm = which == 0 ? kLLDefNorm : (which == 1 ? kOFDefNorm : kMLDefNorm);
    const uint32_t defMax = which == 0 ? 35u : (which == 1 ? 28u : 52u);
    const uint32_t alpha = which == 0 ? 36u : (which == 1 ? 32u : 53u);
    uint32_t maxSym = 0, maxCount = 0, present = 0;
    for (uint32_t s = 0; s < alpha; s++) if (T.count[s]) { maxSym = s; present++; if (T.count[s] > maxCount) maxCount = T.count[s]; }
    T.maxSym = maxSym;
    if (maxCount == nbSeq) {                                   // one code only -> RLE table (1 byte)
        uint32_t sym = maxSym;
        T.mode = 1; T.tableLog = 0; T.descSize = 1; T.desc[0] = (uint8_t)sym; T.tabMaxSym = sym;
        T.state[0] = 0; T.tt[sym].deltaNbBits = 0; T.tt[sym].deltaFindState = 0;
        return;
    }
    // candidate: FSE-compressed table
    uint32_t tl = gc_hibit32(nbSeq - 1u) >= 2u ? gc_hibit32(nbSeq - 1u) - 2u : 0u;     // FSE_optimalTableLog flavour
    { uint32_t minBits = min(gc_hibit32(nbSeq) + 1u, gc_hibit32(maxSym) + 2u); if (tl < minBits) tl = minBits; }
    while ((1u << tl) < present) tl++;
    if (tl < 5u) tl = 5u;
    if (tl > maxLog) tl = maxLog;
    gc_fse_normalize(T.count, maxSym, nbSeq, tl, T.norm);
    // Rare symbols are demoted to a single cell: whatever the state, a count-1 symbol sends it to the same successor, and these
    // are the only points where two walks that started from different states are guaranteed to meet (an FSE step is a monotone
    // map of the state, so walks otherwise keep their distance) -- they are what lets the state chain below be walked in
    // parallel segments.  Cost: < 0.1 bit per sequence on the corpora measured.
    {
        uint32_t freed = 0, big = 0; int bigv = 0;
        for (uint32_t s = 0; s <= maxSym; s++) {
            if (T.norm[s] == 2 || T.norm[s] == 3) { freed += (uint32_t)T.norm[s] - 1u; T.norm[s] = 1; }
            if (T.norm[s] > bigv) { bigv = T.norm[s]; big = s; }
        }
        T.norm[big] = (int16_t)(T.norm[big] + (int)freed);
    }
    // cost comparison in 1/256 bits (free choice; reference: ZSTD_selectEncodingType, zstd_compress_sequences.c:157)
    uint64_t costFse = 0, costDef = 0; bool defOk = maxSym <= defMax;
    for (uint32_t s = 0; s <= maxSym; s++) {
        uint32_t c = T.count[s];
        if (!c) continue;
        costFse += (uint64_t)c * ((tl << 8) - gc_log2_q8((uint32_t)T.norm[s]));
        if (defOk) { int dn = defNorm[s]; costDef += (uint64_t)c * ((defLog << 8) - gc_log2_q8(dn < 1 ? 1u : (uint32_t)dn)); }
    }
    uint32_t descBytes = gc_fse_write_ncount(T.desc, T.norm, maxSym, tl);
    costFse += (uint64_t)descBytes * 8u * 256u;
    if (defOk && costDef <= costFse) {
        T.mode = 0; T.tableLog = defLog; T.descSize = 0; T.tabMaxSym = defMax;
        for (uint32_t s = 0; s <= defMax; s++) T.norm[s] = defNorm[s];
        gc_fse_build_ctable(T.norm, defMax, defLog, T.state, T.tt, T.spread, T.cumul);
    } else {
        T.mode = 2; T.tableLog = tl; T.descSize = descBytes; T.tabMaxSym = maxSym;
        gc_fse_build_ctable(T.norm, maxSym, tl, T.state, T.tt, T.spread, T.cumul);
    }
}

#define SEQ_PHASE(i) do { if (prof && t == 0) { unsigned long long now_ = gc_clock(); atomicAdd(&prof[i], now_ - tprev); tprev = now_; } } while (0)

// ------------------------------------------------------------------------------------------------ K3a codes
// A thread takes SEQ_R consecutive raw records per round (SEQ_N per workgroup); merged sequences collect in an LDS ring and are coded SEQ_R per thread from there, so
// nothing this kernel computes is written to memory and read back (rounds 1-2 wrote the merged sequences out, then read them and their neighbours again).  A round
// crosses four workgroup barriers (the scan of head counts, two around the ring, the scan of run keys) where one record per thread crossed eight.
// One ring entry per merged sequence: ll | ml << 17 | off << 35 (17, 18 and 24 bits: a block has 2^17 bytes, a frame offsets below 2^24) -- a record that continues
// a chain adds its length << 17.
// The three code histograms are kept in SEQ_HIST_REPS copies, side by side per code.  LDS atomics of one wave instruction on one address are carried out one after
// the other, and in text most sequences of a wave share a few codes: with one copy an instruction took as many passes as its most frequent code had lanes.
#ifndef SEQ_HIST_REPS
#define SEQ_HIST_REPS 8u
#endif
#define SEQ_RING (4u * SEQ_N)       // merged sequences the ring holds (> 2 * SEQ_N: up to SEQ_N wait for their batch to fill while a round adds up to SEQ_N)
#define SEQ_ENT(ll, ml, off) ((uint64_t)(ll) | ((uint64_t)(ml) << 17) | ((uint64_t)(off) << 35))
#define SEQ_ENT_OFF(e) ((uint32_t)((e) >> 35))
struct __attribute__((aligned(16))) SeqP2 { uint64_t a, b; };      // two packed sequences: one global_store_dwordx4

extern "C" __global__ void __launch_bounds__(SEQ_T)
gc_zstd_seq_codes_kernel(const GcSeqRaw* __restrict__ seqRaw, const GcBlockMeta* __restrict__ meta,
                   uint64_t* __restrict__ seqPacked,      // out: ll | mlBase << 17 | offBase << 35 per merged sequence
                   uint32_t* __restrict__ seqOff,         // (unused since the ring; kept in the signature for the workspace's sake)
                   uint8_t* __restrict__ codes,           // out: 3 * GC_MAX_SEQ_PER_BLOCK per block (LL, OF, ML)
                   GcSeqHist* __restrict__ hist, uint8_t* __restrict__ seqSec, GcSectionInfo* __restrict__ info,
                   uint32_t frameBlocks,                  // blocks per zstd frame: repeat offsets carry over inside a frame
                   unsigned long long* __restrict__ prof /* optional per-phase cycle sums */)
{
    __shared__ uint32_t sCount[3][64][SEQ_HIST_REPS];   // a lane counts in copy lane % SEQ_HIST_REPS
    __shared__ uint32_t sWave[2][SEQ_T / 64u];
    __shared__ uint64_t sWave64[2][SEQ_T / 64u];
    __shared__ uint64_t sRing[SEQ_RING];
    __shared__ uint8_t sLLCode[64], sMLCode[128];         // kLLCode / kMLCode, staged: a per-lane read of a __constant__ table is a global load
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    const uint32_t nRaw = meta[b].nSeqRaw;
    const GcSeqRaw* R = seqRaw + (uint64_t)b * GC_MAX_SEQ_PER_BLOCK;
    uint64_t* P = seqPacked + (uint64_t)b * GC_MAX_SEQ_PER_BLOCK;
    uint8_t* cLL = codes + (uint64_t)b * 3u * GC_MAX_SEQ_PER_BLOCK;
    uint8_t* cOF = cLL + GC_MAX_SEQ_PER_BLOCK;
    uint8_t* cML = cOF + GC_MAX_SEQ_PER_BLOCK;
    (void)seqOff;
    if (nRaw == 0) { if (t == 0) { seqSec[(uint64_t)b * GC_SEQSEC_STRIDE] = 0; info[b].seqSecSize = 1; info[b].nSeq = 0; } return; }
    for (uint32_t i = t; i < 3u * 64u * SEQ_HIST_REPS; i += SEQ_T) (&sCount[0][0][0])[i] = 0;
    const uint32_t hrep = t & (SEQ_HIST_REPS - 1u);
    if (t < 64u) sLLCode[t] = kLLCode[t];
    if (t < 128u) sMLCode[t] = kMLCode[t];
    unsigned long long tprev = prof ? gc_clock() : 0ull;

    // virtual history of the repeat offsets: index -1 -> offset 1, -2 -> 4 (start state {1,4,8}, zstd_internal.h:65) in the first block of a
    // frame.  In later blocks the decoder arrives with the history the previous block left behind; this block is coded
    // without knowing it (blocks stay independent units of work): the virtual history is "unknown" (0, never equal to
    // an offset), so no repeat code refers to it.  rep1 = previous offset and rep2 = offset before the current run hold
    // for the decoder whatever the unknown part was, because every code emitted below moves exactly those two slots.
    const bool firstInFrame = (b % frameBlocks) == 0u;
    const uint32_t virt1 = firstInFrame ? 1u : 0u, virt2 = firstInFrame ? 4u : 0u;
    uint32_t nMerged = 0, nCoded = 0;        // merged sequences in the ring so far / coded so far (uniform)
    uint32_t par = 0, par64 = 0;             // which half of sWave / sWave64 the next scan takes
    uint32_t carryOff = virt1;               // offset of the last coded sequence
    uint64_t carryPair = (1ull << 32) | virt2;   // (start index + 2 of the run of equal offsets that holds the last coded sequence, offset in front of that run)

    // S2 on the SEQ_N sequences from nCoded on (or the last few), SEQ_R consecutive ones per thread: repeat offsets as scans, codes, histograms.
    // (nCoded is a multiple of SEQ_N in every call: only the block's last batch is short.  `whole`: count == SEQ_N, known where the call is written -- every thread
    // has SEQ_R sequences and the per-sequence conditions fold away.)
    auto code_batch = [&](uint32_t count, auto whole) {
        const uint32_t j0 = nCoded + t * SEQ_R;
        const uint32_t mine = decltype(whole)::value ? SEQ_R : (t * SEQ_R < count ? min(SEQ_R, count - t * SEQ_R) : 0u);
        uint64_t e[SEQ_R], keyIn[SEQ_R]; uint32_t prevOff[SEQ_R];
        uint32_t pOff = carryOff;
        if (mine && t) pOff = SEQ_ENT_OFF(sRing[(j0 - 1u) & (SEQ_RING - 1u)]);
        // a run of equal offsets starts at j: key = (j + 2, the offset in front of the run); the scan hands every j the key of its run.  Keys grow with j, so the
        // maximum over a thread's sequences is the last key among them: a thread scans its own, the workgroup the threads' last keys.
        uint64_t run = 0;
#pragma unroll
        for (uint32_t r = 0; r < SEQ_R; r++) {
            e[r] = 0; prevOff[r] = pOff; keyIn[r] = run;
            if (r < mine) {
                e[r] = sRing[(j0 + r) & (SEQ_RING - 1u)];
                const uint32_t off = SEQ_ENT_OFF(e[r]);
                if (off != pOff) run = (((uint64_t)(j0 + r + 2u)) << 32) | pOff;
                pOff = off;
            }
        }
        uint64_t tot;
        uint64_t front = seq_excl_maxscan64(run, sWave64, par64, &tot);       // ... of the run that holds the sequence in front of this thread's first
        if (carryPair > front) front = carryPair;
        uint32_t packLL = 0, packOF = 0, packML = 0; uint64_t pk[SEQ_R];
#pragma unroll
        for (uint32_t r = 0; r < SEQ_R; r++) {
            pk[r] = 0;
            if (r < mine) {
                const uint32_t j = j0 + r;
                const uint64_t pairPrev = keyIn[r] > front ? keyIn[r] : front;      // ... of the run that holds j - 1
                const uint32_t ll = (uint32_t)e[r] & 0x1FFFFu, ml = (uint32_t)(e[r] >> 17) & 0x3FFFFu, off = SEQ_ENT_OFF(e[r]);
                const uint32_t rep1 = prevOff[r], rep2 = (uint32_t)pairPrev;
                uint32_t offBase;
                if (ll != 0u) offBase = (off == rep1) ? 1u : ((off == rep2) ? 2u : off + 3u);
                else offBase = (off == rep2) ? 1u : ((rep1 > 1u && off == rep1 - 1u) ? 3u : off + 3u);
                const uint32_t mlBase = ml - 3u;
                const uint32_t llc = ll > 63u ? gc_hibit32(ll) + 19u : sLLCode[ll], mlc = mlBase > 127u ? gc_hibit32(mlBase) + 36u : sMLCode[mlBase], ofc = gc_hibit32(offBase);
                packLL |= llc << (8u * r); packOF |= ofc << (8u * r); packML |= mlc << (8u * r);
                atomicAdd(&sCount[0][llc][hrep], 1u); atomicAdd(&sCount[1][ofc][hrep], 1u); atomicAdd(&sCount[2][mlc][hrep], 1u);
                pk[r] = (uint64_t)ll | ((uint64_t)mlBase << 17) | ((uint64_t)offBase << 35);   // ll, mlBase, offBase
#ifdef HIPEMU
                if (getenv("GC_TRACE")) fprintf(stderr, "E %u ofv=%u ml=%u ll=%u off=%u rep1=%u rep2=%u\n", j, offBase, ml, ll, off, rep1, rep2);
#endif
            }
        }
        if (mine == SEQ_R) {                 // whole: SEQ_R code bytes per table in one store (the tables' bases are only 2-byte aligned), the packed words 16 bytes at a time
            __builtin_memcpy(cLL + j0, &packLL, SEQ_R); __builtin_memcpy(cOF + j0, &packOF, SEQ_R); __builtin_memcpy(cML + j0, &packML, SEQ_R);
#pragma unroll
            for (uint32_t r = 0; r < SEQ_R; r += 2u) { SeqP2 v; v.a = pk[r]; v.b = pk[r + 1u]; *(SeqP2*)(P + j0 + r) = v; }
        } else {
#pragma unroll
            for (uint32_t r = 0; r < SEQ_R; r++)
                if (r < mine) { cLL[j0 + r] = (uint8_t)(packLL >> (8u * r)); cOF[j0 + r] = (uint8_t)(packOF >> (8u * r)); cML[j0 + r] = (uint8_t)(packML >> (8u * r)); P[j0 + r] = pk[r]; }
        }
        if (tot > carryPair) carryPair = tot;
        carryOff = SEQ_ENT_OFF(sRing[(nCoded + count - 1u) & (SEQ_RING - 1u)]);
        nCoded += count;
    };

    // this thread's records of a round and the record in front of them (requested a round ahead)
    auto load_records = [&](uint32_t i0, GcSeqRaw (&r)[SEQ_R], GcSeqRaw& q) {
#pragma unroll
        for (uint32_t k = 0; k < SEQ_R; k++) r[k].litRank = r[k].offml = 0;
        q.litRank = q.offml = 0;
        if (i0 >= nRaw) return;
        if (i0 + SEQ_R <= nRaw) {           // (16 bytes at a time: a block's records start 16-byte aligned, GC_MAX_SEQ_PER_BLOCK is even)
#pragma unroll
            for (uint32_t k = 0; k < SEQ_R; k += 2u) {
                const GcU4 v = *(const GcU4*)(R + i0 + k);
                r[k].litRank = v.x; r[k].offml = v.y; r[k + 1u].litRank = v.z; r[k + 1u].offml = v.w;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < SEQ_R; k++) if (i0 + k < nRaw) r[k] = R[i0 + k];
        }
        if (i0) q = R[i0 - 1u];
    };
    GcSeqRaw rNext[SEQ_R], qNext;
    load_records(t * SEQ_R, rNext, qNext);
    for (uint32_t tb = 0; tb < nRaw; tb += SEQ_N) {
        // ---- S1: merge chains of capped matches.  Head = first record of a run with equal offset and litLength 0; the records behind it
        //      add their lengths to it (a chain may run on into the next thread's records or the next round's: the ring's last sequence stays open until then)
        const uint32_t i0 = tb + t * SEQ_R;
        const bool wholeRound = tb + SEQ_N <= nRaw;       // (uniform)
        uint32_t ll[SEQ_R], off[SEQ_R], ml[SEQ_R]; bool valid[SEQ_R], head[SEQ_R];
        uint32_t nHead = 0;
        {
            uint32_t prevRank = qNext.litRank, prevOff = qNext.offml >> 8;      // (both 0 in front of record 0, which is a head whatever they are)
#pragma unroll
            for (uint32_t k = 0; k < SEQ_R; k++) {
                const uint32_t i = i0 + k;
                valid[k] = wholeRound || i < nRaw;
                ll[k] = rNext[k].litRank - prevRank; off[k] = rNext[k].offml >> 8; ml[k] = rNext[k].offml & 0xFFu;
                head[k] = valid[k] && (i == 0u || ll[k] != 0u || off[k] != prevOff);
                nHead += head[k] ? 1u : 0u;
                prevRank = rNext[k].litRank; prevOff = off[k];
            }
        }
        load_records(i0 + SEQ_N, rNext, qNext);
        uint32_t tot;
        const uint32_t before = seq_excl_scan(nHead, sWave, par, &tot);
        // the thread folds its own records: a sequence goes into the ring when the next head closes it (or the thread's records end: it may still grow); the
        // records in front of the thread's first head belong to the sequence of the head in front of them, in another thread's hands or an earlier round's
        uint32_t slot = nMerged + before, leadMl = 0; bool open = false; uint64_t cur = 0;
#pragma unroll
        for (uint32_t k = 0; k < SEQ_R; k++) {
            if (head[k]) { if (open) { sRing[slot & (SEQ_RING - 1u)] = cur; slot++; } cur = SEQ_ENT(ll[k], ml[k], off[k]); open = true; }
            else if (valid[k]) { if (open) cur += (uint64_t)ml[k] << 17; else leadMl += ml[k]; }
        }
        if (open) sRing[slot & (SEQ_RING - 1u)] = cur;
        __syncthreads();
        if (leadMl) atomicAdd((unsigned long long*)&sRing[(nMerged + before - 1u) & (SEQ_RING - 1u)], (unsigned long long)leadMl << 17);
        nMerged += tot;
        __syncthreads();
        // ---- S2 whenever SEQ_N sequences are complete (the last one in the ring may still grow)
        while (nMerged - nCoded > SEQ_N) code_batch(SEQ_N, std::true_type());
    }
    SEQ_PHASE(0);         // merge (and the batches coded on the way)
    while (nCoded < nMerged) code_batch(nMerged - nCoded < SEQ_N ? nMerged - nCoded : SEQ_N, std::false_type());
    __syncthreads();
    for (uint32_t i = t; i < 3u * 64u; i += SEQ_T) {
        uint32_t n = 0;
        for (uint32_t k = 0; k < SEQ_HIST_REPS; k++) n += sCount[i >> 6][i & 63u][k];
        hist[b].count[i >> 6][i & 63u] = n;
    }
    if (t == 0) info[b].nSeq = nMerged;
    SEQ_PHASE(1);         // repcodes + codes + histograms
}

// ------------------------------------------------------------------------------------------------ K3b tables
// workgroup (one wave) bt = 3 * block + table; table 0 LL, 1 OF, 2 ML
extern "C" __global__ void __launch_bounds__(64)
gc_zstd_seq_tables_kernel(const GcSeqHist* __restrict__ hist, const GcSectionInfo* __restrict__ info, GcSeqTabG* __restrict__ tabs,
                          unsigned long long* __restrict__ prof)
{
    __shared__ SeqTab T;
    const uint32_t t = threadIdx.x, b = blockIdx.x / 3u, which = blockIdx.x % 3u;
    const uint32_t nSeq = info[b].nSeq;
    if (nSeq == 0u) return;
    unsigned long long tprev = prof ? gc_clock() : 0ull;
    T.count[t] = hist[b].count[which][t];
    T.norm[t] = 0;
    if (t == 0) T.finalState = 0;
    gc_wave_sync();
    if (t == 0) seq_build_table(T, (int)which, nSeq);
    gc_wave_sync();
    GcSeqTabG& G = tabs[blockIdx.x];
    for (uint32_t i = t; i < 512u; i += 64u) G.state[i] = T.state[i];
    G.tt[t] = T.tt[t];
    G.norm[t] = T.norm[t];
    for (uint32_t i = t; i < 96u; i += 64u) G.desc[i] = T.desc[i];
    if (t == 0) { G.descSize = T.descSize; G.mode = T.mode; G.tableLog = T.tableLog; G.maxSym = T.maxSym; G.tabMaxSym = T.tabMaxSym; G.finalState = 0; }
    SEQ_PHASE(2);         // tables
}

// ------------------------------------------------------------------------------------------------ K3c chains
// One wave walks table `which`'s FSE state backwards over the block's sequences (last sequence first = processing index 0).
//      The walk is serial through the state, but walks that started from different states meet at the next symbol whose
//      normalised count is 1 (every state has the same successor there; the table builder makes sure such symbols
//      exist).  So the 64 lanes of the wave walk 64 consecutive segments of 64 sequences at once: a lane first runs
//      ahead of its segment from the nearest such meeting point before it (no output), then its own segment.  Afterwards every
//      segment's start state is compared with its predecessor's final state; a segment that started wrong is walked again
//      from the right state, only until it rejoins the states it went through before (kept at every 8th symbol), and this repeats until
//      nothing changes (each round settles at least one more segment, so the result is exactly the serial walk).
// Output: nbBits << 10 | state BEFORE the symbol (10 bits): the bits to emit are its low nbBits.  Symbol k of segment `lane` of a tile is processing
// index u = 64 * lane + k; it is stored at SEQ_ST_IDX(u) = 256 * (lane / 4) + 4 * k + lane % 4, i.e. the 256 symbols of four neighbouring segments
// share 512 bytes: a step of the walk writes 8 bytes per group of four lanes, sixteen steps fill a line, and the 256 sequences a pack
// workgroup takes per round are four whole lines (in segment-major order the same round touched 64 lines: 3.7 GB fetched for 0.4 GB of states).
#define SEQ_ST_IDX(u) (((u) & ~255u) + (((u) & 63u) << 2) + (((u) >> 6) & 3u))
extern "C" __global__ void __launch_bounds__(64)
gc_zstd_seq_chain_kernel(const uint8_t* __restrict__ codes, const GcSectionInfo* __restrict__ info, GcSeqTabG* __restrict__ tabs,
                         uint16_t* __restrict__ states,   // out: 3 * GC_SEQ_ST_STRIDE per block (LL, OF, ML)
                         unsigned long long* __restrict__ prof)
{
    __shared__ uint16_t sState[512];
    __shared__ GcFseSym sTT[64];
    __shared__ uint8_t  tCode[SEQ_CHAIN_TILE + SEQ_CHAIN_TILE / SEQ_CHAIN_SEG + 3u];
    __shared__ uint64_t sMeet[SEQ_CHAIN_TILE / 64u];
    __shared__ uint16_t sChk[64u * (SEQ_CHAIN_SEG / SEQ_CHK + 1u)];        // [lane][checkpoint], row stride 9 half-words
    const uint32_t t = threadIdx.x, lane = t, b = blockIdx.x / 3u, which = blockIdx.x % 3u;
    const uint32_t nSeq = info[b].nSeq;
    if (nSeq == 0u) return;
    GcSeqTabG& G = tabs[blockIdx.x];
    if (G.mode == 1u) return;                                 // RLE table: no state bits at all (the pack kernel knows)
    unsigned long long tprev = prof ? gc_clock() : 0ull;
    unsigned long long tsub = 0;
#define SEQ_SUB(i) do { if (prof && t == 0) { unsigned long long now_ = gc_clock(); if (tsub) atomicAdd(&prof[i], now_ - tsub); tsub = now_; } } while (0)
    const uint8_t* C = codes + ((uint64_t)b * 3u + which) * GC_MAX_SEQ_PER_BLOCK;
    uint16_t* S = states + ((uint64_t)b * 3u + which) * GC_SEQ_ST_STRIDE;
    for (uint32_t i = lane; i < 512u; i += 64u) sState[i] = G.state[i];
    sTT[lane] = G.tt[lane];
    const uint32_t L = G.tableLog;
    int nv = 0;
    if (lane <= G.tabMaxSym) nv = G.norm[lane];
    const uint64_t resetMask = __ballot(nv == 1 || nv == -1);    // symbols that send every state to the same successor
    gc_wave_sync();
    uint32_t carry = 0;                               // state after the last sequence of the previous tile
    for (uint32_t tb = 0; tb < nSeq; tb += SEQ_CHAIN_TILE) {
        const uint32_t tileLen = min(SEQ_CHAIN_TILE, nSeq - tb);
        if (prof && t == 0) tsub = gc_clock();
        // stage the codes (independent loads, eight in flight per lane), then per 64 sequences one mask of the positions
        // that hold a count-1 symbol ("meeting points")
        // (tile element u is sequence nSeq - 1 - (tb + u): sixteen elements per lane and load, read upwards in memory and stored back to front)
        for (uint32_t u16 = lane * 16u; u16 < tileLen; u16 += 64u * 16u) {
            const uint32_t jTop = nSeq - 1u - (tb + u16);         // sequence of element u16; the lane's elements are jTop, jTop - 1, ...
            if (u16 + 16u <= tileLen) {
                GcU4 v; __builtin_memcpy(&v, C + (jTop - 15u), 16);
                const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (uint32_t i = 0; i < 16u; i++) tCode[SEQ_TC(u16 + i)] = (uint8_t)(w[(15u - i) >> 2] >> (((15u - i) & 3u) * 8u));
            } else
                for (uint32_t i = 0; u16 + i < tileLen; i++) tCode[SEQ_TC(u16 + i)] = C[jTop - i];
        }
        gc_wave_sync();
        SEQ_SUB(5);
        for (uint32_t k = 0; k < tileLen; k += 64u) {
            const uint32_t u = k + lane;
            const bool isR = u < tileLen && ((resetMask >> tCode[SEQ_TC(u)]) & 1ull) != 0ull;
            const uint64_t bal = __ballot(isR);
            if (lane == 0u) sMeet[k >> 6] = bal;
        }
        gc_wave_sync();
        const uint32_t nSegs = (tileLen + SEQ_CHAIN_SEG - 1u) / SEQ_CHAIN_SEG;      // <= 64: lane i walks segment i
        const uint32_t u0 = lane * SEQ_CHAIN_SEG, u1 = min(u0 + SEQ_CHAIN_SEG, tileLen);
        uint32_t first = u0;                          // first index of the segment that emits bits
        uint32_t st0 = carry;
        if (lane < nSegs) {
            if (tb + u0 == 0u) { st0 = gc_fse_init_state(sState, sTT[tCode[SEQ_TC(0)]]); S[0] = 0; first = 1u; }   // FSE_initCState2: no bits
            else if (lane != 0u) {
                // run ahead from the nearest meeting point in the SEQ_WARM_SEGS segments before this one (from there the
                // state is exact whatever it was before); if there is none, from SEQ_WARM_SEGS segments back (a guess)
                uint32_t w = lane > SEQ_WARM_SEGS ? (lane - SEQ_WARM_SEGS) * SEQ_CHAIN_SEG : 0u;
                for (uint32_t c = lane; c-- > 0u && c + SEQ_WARM_SEGS >= lane; ) {
                    const uint64_t m = sMeet[c];
                    if (m) { w = c * 64u + 63u - (uint32_t)__clzll((long long)m); break; }
                }
                if (tb + w == 0u) { st0 = gc_fse_init_state(sState, sTT[tCode[SEQ_TC(0)]]); w = 1u; }                   // exact, not a guess
                else st0 = 1u << L;
                if (w < u0) {                              // the symbol's table entry does not depend on the state: fetched one
                    GcFseSym sy = sTT[tCode[SEQ_TC(w)]];      // step ahead, so a step costs one dependent LDS read, not three
                    for (; w < u0; w++) {
                        const GcFseSym nx = sTT[tCode[SEQ_TC(w + 1u < u0 ? w + 1u : w)]];
                        const uint32_t nb = (st0 + sy.deltaNbBits) >> 16;
                        st0 = sState[(st0 >> nb) + (uint32_t)sy.deltaFindState];
                        sy = nx;
                    }
                }
            }
        }
        SEQ_SUB(6);
        uint32_t fin = st0;
        bool redo = lane < nSegs;
        bool firstPass = true;
        uint16_t* chk = sChk + lane * (SEQ_CHAIN_SEG / SEQ_CHK + 1u);
        uint16_t* Sk = S + tb + ((lane >> 2) << 8) + (lane & 3u);      // symbol k of this lane's segment -> Sk[4 * k]
#ifdef HIPEMU
        uint32_t dbgRounds = 0, dbgRedo = 0;
#endif
        for (;;) {
            if (redo) {
                uint32_t state = st0, u = first;
                GcFseSym sy = sTT[tCode[SEQ_TC(u < u1 ? u : u1 - 1u)]];
                for (; u < u1; u++) {
                    const uint32_t k = u - u0;
                    if ((k & (SEQ_CHK - 1u)) == 0u) {
                        if (!firstPass && chk[k / SEQ_CHK] == (uint16_t)state) break;     // rejoined: the rest is what it was
                        chk[k / SEQ_CHK] = (uint16_t)state;
                    }
                    const GcFseSym nx = sTT[tCode[SEQ_TC(u + 1u < u1 ? u + 1u : u)]];
                    const uint32_t nb = (state + sy.deltaNbBits) >> 16;
                    Sk[4u * k] = (uint16_t)((nb << 10) | (state & 0x3FFu));
                    state = sState[(state >> nb) + (uint32_t)sy.deltaFindState];
                    sy = nx;
                }
                if (u == u1) fin = state;                 // walked to the end: the final state may have changed
            }
            firstPass = false;
            const uint32_t prevFin = __shfl_up(fin, 1);
            redo = lane != 0u && lane < nSegs && prevFin != st0;
            if (redo) st0 = prevFin;
#ifdef HIPEMU
            dbgRounds++; dbgRedo += (uint32_t)__popcll(__ballot(redo));
#endif
            if (!__any(redo)) break;
        }
#ifdef HIPEMU
        if (getenv("GC_TRACE_CHAIN") && lane == 0) fprintf(stderr, "chain table=%u tile=%u len=%u L=%u rounds=%u redone=%u\n", which, tb, tileLen, L, dbgRounds, dbgRedo);
#endif
        carry = __shfl(fin, (int)(nSegs - 1u));
        gc_wave_sync();
        SEQ_SUB(7);
    }
    if (lane == 0u) G.finalState = carry;
    SEQ_PHASE(3);         // state chains
}

// ------------------------------------------------------------------------------------------------ K3d pack
struct SeqPackLds { uint32_t wave[2][SEQ_T / 64u]; uint32_t tile[SEQ_TILE_WORDS]; uint32_t mode[3], log[3], fin[3], desc[3]; uint8_t llBits[40], mlBits[56]; };      // the calling kernel's LDS

// One round's input of a thread: SEQ_R sequences, requested a round ahead.  Wave w takes the elements tb + 64 * (SEQ_R * w + s) + lane, s < SEQ_R, of a round (element u is
// sequence nSeq - 1 - u): for every s the wave reads 64 neighbouring packed words and code bytes, and its SEQ_R states of one table lie side by side in SEQ_ST_IDX's order,
// which groups four 64-element segments per 512 bytes -- one load per table and lane, whole lines per wave.
#if SEQ_R == 4u
typedef uint64_t SeqStWord;
#elif SEQ_R == 2u
typedef uint32_t SeqStWord;
#else
#error "SEQ_R is 2 or 4: the states of SEQ_R segments are one aligned load"
#endif
struct SeqPackIn { uint64_t pk[SEQ_R]; uint32_t codes[SEQ_R]; SeqStWord st[3]; };     // codes: LL | OF << 8 | ML << 16; st: LL, OF, ML

// block b of the workspace, whose content is blockLen bytes long (a section that does not stay below that is given up: the block is stored raw)
__device__ __forceinline__ void seq_pack_block(const uint64_t* __restrict__ seqPacked, const uint8_t* __restrict__ codes, const uint16_t* __restrict__ states,
                                               const GcSeqTabG* __restrict__ tabs, uint8_t* __restrict__ seqSec, GcSectionInfo* __restrict__ info,
                                               const uint32_t b, const uint32_t blockLen, unsigned long long* __restrict__ prof, SeqPackLds& L)
{
    uint32_t* const sTile = L.tile;
    uint32_t* const sMode = L.mode; uint32_t* const sLog = L.log; uint32_t* const sFinal = L.fin; uint32_t* const sDesc = L.desc;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t nSeq = info[b].nSeq;
    if (nSeq == 0u) return;                                   // (the codes kernel has written the one-byte section)
    unsigned long long tprev = prof ? gc_clock() : 0ull;
    const uint64_t* P = seqPacked + (uint64_t)b * GC_MAX_SEQ_PER_BLOCK;
    const uint8_t* cLL = codes + (uint64_t)b * 3u * GC_MAX_SEQ_PER_BLOCK;
    const uint8_t* cOF = cLL + GC_MAX_SEQ_PER_BLOCK;
    const uint8_t* cML = cOF + GC_MAX_SEQ_PER_BLOCK;
    const uint16_t* stLL = states + (uint64_t)b * 3u * GC_SEQ_ST_STRIDE;
    const uint16_t* stOF = stLL + GC_SEQ_ST_STRIDE;
    const uint16_t* stML = stOF + GC_SEQ_ST_STRIDE;
    const GcSeqTabG* G = tabs + (uint64_t)b * 3u;
    uint8_t* out = seqSec + (uint64_t)b * GC_SEQSEC_STRIDE;
    if (t < 3u) { sMode[t] = G[t].mode; sLog[t] = G[t].tableLog; sFinal[t] = G[t].finalState; sDesc[t] = G[t].descSize; }
    if (t < 36u) L.llBits[t] = kLLBits[t];                    // (staged: a per-lane read of a __constant__ table is a global load)
    if (t >= 64u && t < 64u + 53u) L.mlBits[t - 64u] = kMLBits[t - 64u];
    __syncthreads();

    // ---- section header (zstd_compress.c:2939-2953 nbSeq; modes byte; table descriptions LL, OF, ML)
    uint32_t hdrLen;
    {
        uint32_t h = nSeq < 128u ? 1u : (nSeq < 0x7F00u ? 2u : 3u);
        hdrLen = h + 1u + sDesc[0] + sDesc[1] + sDesc[2];
        if (t == 0) {
            if (h == 1u) out[0] = (uint8_t)nSeq;
            else if (h == 2u) { out[0] = (uint8_t)((nSeq >> 8) + 0x80u); out[1] = (uint8_t)nSeq; }
            else { out[0] = 0xFF; out[1] = (uint8_t)(nSeq - 0x7F00u); out[2] = (uint8_t)((nSeq - 0x7F00u) >> 8); }
            out[h] = (uint8_t)((sMode[0] << 6) | (sMode[1] << 4) | (sMode[2] << 2));
            uint32_t p = h + 1u;
            for (int k = 0; k < 3; k++) for (uint32_t i = 0; i < sDesc[k]; i++) out[p++] = G[k].desc[i];
        }
    }
    const bool rleLL = sMode[0] == 1u, rleOF = sMode[1] == 1u, rleML = sMode[2] == 1u;

    const uint32_t uWave = 64u * SEQ_R * wave + lane;         // this thread's elements of a round: tb + uWave + 64 * s
    const uint32_t stWave = ((64u * SEQ_R * wave) & ~255u) + 4u * lane + ((SEQ_R * wave) & 3u);      // SEQ_ST_IDX of the first of them (behind tb)
    auto fetch = [&](uint32_t tb, SeqPackIn& in) {
#pragma unroll
        for (uint32_t s = 0; s < SEQ_R; s++) {
            const uint32_t u = tb + uWave + 64u * s;
            in.pk[s] = 0; in.codes[s] = 0;
            if (u < nSeq) { const uint32_t j = nSeq - 1u - u; in.pk[s] = P[j]; in.codes[s] = (uint32_t)cLL[j] | ((uint32_t)cOF[j] << 8) | ((uint32_t)cML[j] << 16); }
        }
        in.st[0] = in.st[1] = in.st[2] = 0;
        if (tb + uWave < nSeq) {           // (a table in RLE mode has no states: the chain kernel wrote none)
            if (!rleLL) in.st[0] = *(const SeqStWord*)(stLL + tb + stWave);
            if (!rleOF) in.st[1] = *(const SeqStWord*)(stOF + tb + stWave);
            if (!rleML) in.st[2] = *(const SeqStWord*)(stML + tb + stWave);
        }
    };

    // ---- pack the bitstream, last sequence first
    const uint32_t limit = min(blockLen, (uint32_t)GC_SEQSEC_STRIDE - 64u);
    uint8_t* so = out + hdrLen;
    uint32_t carryBits = 0, carryVal = 0, outBytes = 0, par = 0; bool overflow = false;
    SeqPackIn nx;
    fetch(0u, nx);
    for (uint32_t tb = 0; tb < nSeq && !overflow; tb += SEQ_N) {
        const uint32_t tileWords = (min(SEQ_N, nSeq - tb) * 80u) / 32u + 8u;       // what this round's sequences can fill
        for (uint32_t i = t; i < tileWords; i += SEQ_T) sTile[i] = 0;
        const SeqPackIn in = nx;
        if (tb + SEQ_N < nSeq) fetch(tb + SEQ_N, nx);
        uint64_t a[SEQ_R], c[SEQ_R]; uint32_t na[SEQ_R], nc[SEQ_R], incl[SEQ_R];
        uint32_t waveBits = 0;
#pragma unroll
        for (uint32_t s = 0; s < SEQ_R; s++) {
            const uint32_t u = tb + uWave + 64u * s;
            a[s] = 0; c[s] = 0; na[s] = 0; nc[s] = 0;
            if (u < nSeq) {
                const uint64_t pk = in.pk[s];
                const uint32_t ll = (uint32_t)(pk & 0x1FFFFu), mlBase = (uint32_t)((pk >> 17) & 0x3FFFFu), offBase = (uint32_t)(pk >> 35);
                const uint32_t llc = in.codes[s] & 0xFFu, ofc = (in.codes[s] >> 8) & 0xFFu, mlc = in.codes[s] >> 16;
                if (u != 0u) {
                    const uint32_t so_ = (uint32_t)(in.st[1] >> (16u * s)) & 0xFFFFu, sm = (uint32_t)(in.st[2] >> (16u * s)) & 0xFFFFu, sl = (uint32_t)(in.st[0] >> (16u * s)) & 0xFFFFu;
                    a[s] |= (uint64_t)(so_ & ((1u << (so_ >> 10)) - 1u)) << na[s]; na[s] += so_ >> 10;     // low nbBits of the state (stored whole)
                    a[s] |= (uint64_t)(sm & ((1u << (sm >> 10)) - 1u)) << na[s]; na[s] += sm >> 10;
                    a[s] |= (uint64_t)(sl & ((1u << (sl >> 10)) - 1u)) << na[s]; na[s] += sl >> 10;
                }
                { uint32_t nb = L.llBits[llc]; a[s] |= (uint64_t)(ll & ((1u << nb) - 1u)) << na[s]; na[s] += nb; }
                { uint32_t nb = L.mlBits[mlc]; c[s] |= (uint64_t)(mlBase & ((1u << nb) - 1u)); nc[s] += nb; }
                { c[s] |= (uint64_t)(offBase & ((1u << ofc) - 1u)) << nc[s]; nc[s] += ofc; }
            }
            // bit offsets: the wave's elements are ordered s first, lane second -- a wave scan per s, the totals of the s in front added
            incl[s] = gc_wave_incl_sum_dpp(na[s] + nc[s]) + waveBits;
            waveBits = gc_readlane(incl[s], 63u);
        }
        // ... and one barrier for the waves' totals (it also stands between the zeroing of the tile and the fields OR-ed into it)
        uint32_t* const W = L.wave[par]; par ^= 1u;
        if (lane == 63u) W[wave] = waveBits;
        __syncthreads();
        uint32_t before = carryBits, tileBits = 0;
        for (uint32_t w = 0; w < SEQ_T / 64u; w++) { const uint32_t v = W[w]; if (w < wave) before += v; tileBits += v; }
        if (t == 0 && carryBits) atomicOr(&sTile[0], carryVal);
#pragma unroll
        for (uint32_t s = 0; s < SEQ_R; s++) {
            const uint32_t off = before + incl[s] - (na[s] + nc[s]);
            seq_or_bits(sTile, off, a[s], na[s]);
            seq_or_bits(sTile, off + na[s], c[s], nc[s]);
        }
        uint32_t endBits = carryBits + tileBits;
        const bool lastTile = tb + SEQ_N >= nSeq;
        if (lastTile) {
            if (t == 0) {      // final states ML, OF, LL then the closing bit (zstd_compress_sequences.c:372-376)
                uint32_t e = endBits;
                seq_or_bits(sTile, e, sFinal[2] & ((1u << sLog[2]) - 1u), sLog[2]); e += sLog[2];
                seq_or_bits(sTile, e, sFinal[1] & ((1u << sLog[1]) - 1u), sLog[1]); e += sLog[1];
                seq_or_bits(sTile, e, sFinal[0] & ((1u << sLog[0]) - 1u), sLog[0]); e += sLog[0];
                seq_or_bits(sTile, e, 1u, 1u);
            }
            endBits += sLog[0] + sLog[1] + sLog[2] + 1u;
        }
        __syncthreads();
        const uint32_t flush = lastTile ? (endBits + 7u) >> 3 : endBits >> 3;
        if (hdrLen + outBytes + flush > limit) overflow = true;
        else {
            // the round's bytes leave as aligned dwords, single bytes only in front of the first and behind the last of them
            uint8_t* const dst = so + outBytes;
            const uint32_t lead = min(flush, (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & 3u), nWords = (flush - lead) >> 2, tail = lead + 4u * nWords;
            if (t < lead) dst[t] = (uint8_t)(sTile[0] >> (t * 8u));
            for (uint32_t i = t; i < nWords; i += SEQ_T) {
                const uint32_t w = lead ? (uint32_t)((((uint64_t)sTile[i + 1u] << 32) | sTile[i]) >> (lead * 8u)) : sTile[i];
                *(uint32_t*)(dst + lead + 4u * i) = w;
            }
            if (t >= SEQ_T - 4u && tail + (t - (SEQ_T - 4u)) < flush) { const uint32_t i = tail + (t - (SEQ_T - 4u)); dst[i] = (uint8_t)(sTile[i >> 2] >> ((i & 3u) * 8u)); }
            carryBits = endBits & 7u;
            carryVal = lastTile ? 0u : ((sTile[flush >> 2] >> ((flush & 3u) * 8u)) & 0xFFu);
            outBytes += flush;
        }
        __syncthreads();
    }
    SEQ_PHASE(4);         // pack
    if (t == 0) info[b].seqSecSize = overflow ? 0xFFFFFFFFu : hdrLen + outBytes;
}

extern "C" __global__ void __launch_bounds__(SEQ_T)
gc_zstd_seq_pack_kernel(const uint64_t* __restrict__ seqPacked, const uint8_t* __restrict__ codes, const uint16_t* __restrict__ states,
                        const GcSeqTabG* __restrict__ tabs, uint8_t* __restrict__ seqSec, GcSectionInfo* __restrict__ info, uint64_t srcSize,
                        unsigned long long* __restrict__ prof)
{
    __shared__ SeqPackLds L;
    const uint32_t b = blockIdx.x;
    const uint64_t blockBase = (uint64_t)b * GC_ZSTD_BLOCK_MAX;
    const uint32_t blockLen = (uint32_t)((srcSize - blockBase) < GC_ZSTD_BLOCK_MAX ? (srcSize - blockBase) : GC_ZSTD_BLOCK_MAX);
    seq_pack_block(seqPacked, codes, states, tabs, seqSec, info, b, blockLen, prof, L);
}

// K3d of a batch (gc_zstd_batch.h): block b of the workspace holds item b, whose length comes from the item table
extern "C" __global__ void __launch_bounds__(SEQ_T)
gc_zstd_seq_pack_batch_kernel(const uint64_t* __restrict__ seqPacked, const uint8_t* __restrict__ codes, const uint16_t* __restrict__ states,
                              const GcSeqTabG* __restrict__ tabs, uint8_t* __restrict__ seqSec, GcSectionInfo* __restrict__ info,
                              const gc_batch_item* __restrict__ items)
{
    __shared__ SeqPackLds L;
    seq_pack_block(seqPacked, codes, states, tabs, seqSec, info, blockIdx.x, items[blockIdx.x].src_size, nullptr, L);
}

// ------------------------------------------------------------------------------------------------ the wave scans of gc_device.h, for the tests
// (gc_api.hip gc_test_wave_scans, test builds only) one wave per 64 values
extern "C" __global__ void __launch_bounds__(64)
gc_wave_scan_test_kernel(const uint32_t* __restrict__ v, const uint64_t* __restrict__ keys, uint32_t* __restrict__ sum, uint32_t* __restrict__ mx, uint64_t* __restrict__ mx64)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    sum[i] = gc_wave_incl_sum_dpp(v[i]);
    mx[i] = gc_wave_incl_max_dpp(v[i]);
    mx64[i] = gc_wave_incl_max64_dpp(keys[i]);
}
