// gc_zstd_frame.hip -- K4/K5: frame planning and assembly.
//
// Every run of `frameBlocks` blocks becomes one single-segment zstd frame (magic, frame header descriptor, frame content
// size, then per block a 3-byte header + payload) -- ZSTD_writeFrameHeader (C/zstd/zstd_compress.c:4695-4745), block header
// `last | type<<1 | size<<3` (:4655-4658), raw-block fallback when the sections do not beat the input
// (ZSTD_noCompressBlock, zstd_compress_internal.h:650; decision :3033-3035).  frameBlocks = 1 (block-local match finder):
// every block is its own frame.  The reference decoder accepts any number of concatenated frames
// (CPP/7zip/Compress/ZstdDecoder.cpp:145-158), which is what makes frames independent units for the GPU and, one level
// up, for range-splitting across GPUs.
//
// Content checksums (gc_ctx_set_option GC_OPT_ZSTD_CHECKSUM; what ZSTD_c_checksumFlag = 1 writes, ZSTD_writeEpilogue zstd_compress.c:5225-5232): K0x
// (gc_xxh64.hip) has left XXH64 of every frame's content in `hash`; K4 counts 4 more bytes behind the last block of every frame, K5 sets
// Content_Checksum_Flag in the frame header descriptor and the workgroup of that block writes the low 32 bits there, little endian.
#include "gc_common.h"
#include "gc_device.h"
#include "gc_xxh64.h"      // K0x: gc_zstd_xxh64_kernel

#define FRAME_T 256u

__device__ __forceinline__ uint32_t frame_hdr_size(uint32_t frameLen) { return 5u + (frameLen < 256u ? 1u : (frameLen < 65536u + 256u ? 2u : 4u)); }
// content length of the frame that block b belongs to
__device__ __forceinline__ uint32_t frame_len_of(uint32_t b, uint32_t frameBlocks, uint64_t srcSize)
{
    const uint64_t fb = (uint64_t)frameBlocks * GC_ZSTD_BLOCK_MAX;
    const uint64_t start = (uint64_t)(b / frameBlocks) * fb;
    return (uint32_t)((srcSize - start) < fb ? (srcSize - start) : fb);
}
// bytes a block of blockLen content bytes takes in the output -- hdr bytes of frame header in front, the 3-byte block header, the two sections or, where they do not
// beat it, the content itself (comp = 0), tail bytes of checksum behind
__device__ __forceinline__ uint32_t frame_block_size(const GcSectionInfo si, uint32_t blockLen, uint32_t hdr, uint32_t tail, uint32_t& comp)
{
    const uint64_t payload = (uint64_t)si.litSecSize + si.seqSecSize;
    comp = (si.seqSecSize != 0xFFFFFFFFu && payload < blockLen) ? 1u : 0u;
    return hdr + 3u + (comp ? (uint32_t)payload : blockLen) + tail;
}
// exclusive prefix sum of `size` over the 1024 threads of the workgroup (sWave: 16 words of LDS; both barriers inside); *all = the sum
__device__ __forceinline__ uint32_t frame_excl_scan(uint32_t size, uint32_t* sWave, uint32_t* all)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = gc_wave_incl_sum(size);
    if (lane == 63u) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (uint32_t w = 0; w < 16u; w++) { uint32_t c = sWave[w]; if (w < wave) before += c; sum += c; }
    __syncthreads();
    *all = sum;
    return before + incl - size;
}

// K4: one workgroup; exclusive scan of frame sizes
extern "C" __global__ void __launch_bounds__(1024)
gc_zstd_plan_kernel(const GcSectionInfo* __restrict__ info, uint32_t nBlocks, uint64_t srcSize, uint64_t dstCap, uint32_t frameBlocks,
                    GcFramePlan* __restrict__ plan, uint64_t* __restrict__ result /* [0]=total bytes, [1]=error */,
                    uint32_t seekTable /* 1: a seek table (skippable frame) follows the last frame */,
                    uint32_t checksum /* 1: every frame ends with its content checksum, and the seek table lists them */)
{
    __shared__ uint32_t sWave[16];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t tb = 0; tb < nBlocks; tb += 1024u) {
        const uint32_t b = tb + t;
        uint32_t size = 0, comp = 0;
        if (b < nBlocks) {
            const uint64_t base = (uint64_t)b * GC_ZSTD_BLOCK_MAX;
            const uint32_t blockLen = (uint32_t)((srcSize - base) < GC_ZSTD_BLOCK_MAX ? (srcSize - base) : GC_ZSTD_BLOCK_MAX);
            const uint32_t hdr = (b % frameBlocks) == 0u ? frame_hdr_size(frame_len_of(b, frameBlocks, srcSize)) : 0u;
            const bool last = (b % frameBlocks) == frameBlocks - 1u || b == nBlocks - 1u;
            size = frame_block_size(info[b], blockLen, hdr, (checksum && last) ? 4u : 0u, comp);
        }
        uint32_t all;
        const uint32_t before = frame_excl_scan(size, sWave, &all);
        if (b < nBlocks) { GcFramePlan p; p.off = carry + before; p.size = size; p.compressed = comp; plan[b] = p; }
        carry += all;
    }
    if (t == 0) {
        const uint32_t nFrames = (nBlocks + frameBlocks - 1u) / frameBlocks;
        const uint64_t total = carry + (seekTable ? 8ull + (checksum ? 12ull : 8ull) * nFrames + 9ull : 0ull);
        result[0] = total; result[1] = total > dstCap ? 1u : 0u;
    }
}

// One block of a frame, by the whole workgroup: [frame header] block header, payload (the two sections, or the blockLen content bytes at `s` where K4 chose the raw
// block) [, content checksum].  o = where K4 put the block; first / last: of its frame, whose content is frameLen bytes; hash: the frame's XXH64, or null.
__device__ __forceinline__ void frame_write_block(uint8_t* __restrict__ o, const GcFramePlan p, const GcSectionInfo si, const bool first, const bool last, const uint32_t frameLen,
                                                  const uint32_t blockLen, const uint8_t* __restrict__ s, const uint8_t* __restrict__ ls, const uint8_t* __restrict__ ss,
                                                  const uint64_t* __restrict__ hash)
{
    const uint32_t t = threadIdx.x;
    const uint32_t hs = first ? frame_hdr_size(frameLen) : 0u;
    if (t == 0) {
        if (first) {
            o[0] = 0x28; o[1] = 0xB5; o[2] = 0x2F; o[3] = 0xFD;                     // ZSTD_MAGICNUMBER 0xFD2FB528
            const uint32_t fcsCode = hs == 6u ? 0u : (hs == 7u ? 1u : 2u);
            o[4] = (uint8_t)((fcsCode << 6) | (1u << 5) | (hash ? 1u << 2 : 0u));    // single segment, [content checksum,] no dictID
            if (hs == 6u) o[5] = (uint8_t)frameLen;
            else if (hs == 7u) { uint32_t v = frameLen - 256u; o[5] = (uint8_t)v; o[6] = (uint8_t)(v >> 8); }
            else { o[5] = (uint8_t)frameLen; o[6] = (uint8_t)(frameLen >> 8); o[7] = (uint8_t)(frameLen >> 16); o[8] = (uint8_t)(frameLen >> 24); }
        }
        const uint32_t bsz = p.compressed ? si.litSecSize + si.seqSecSize : blockLen;
        const uint32_t bh = (last ? 1u : 0u) | ((p.compressed ? 2u : 0u) << 1) | (bsz << 3);  // last block, type, size
        o[hs] = (uint8_t)bh; o[hs + 1u] = (uint8_t)(bh >> 8); o[hs + 2u] = (uint8_t)(bh >> 16);
        if (hash && last) {                                                          // the frame's last four bytes (K4 counted them into p.size)
            const uint32_t h = (uint32_t)*hash;
            uint8_t* e = o + p.size - 4u;
            e[0] = (uint8_t)h; e[1] = (uint8_t)(h >> 8); e[2] = (uint8_t)(h >> 16); e[3] = (uint8_t)(h >> 24);
        }
    }
    uint8_t* pay = o + hs + 3u;
    if (p.compressed) {
        for (uint32_t i = t; i < si.litSecSize; i += FRAME_T) pay[i] = ls[i];
        pay += si.litSecSize;
        for (uint32_t i = t; i < si.seqSecSize; i += FRAME_T) pay[i] = ss[i];
    } else {
        for (uint32_t i = t; i < blockLen; i += FRAME_T) pay[i] = s[i];
    }
}

// K5: one workgroup per block writes its frame; with a seek table one more workgroup (blockIdx == nBlocks) writes it:
//   0x184D2A5E | size of the rest | per frame { compressed size, decompressed size [, checksum] } | number of frames | descriptor | 0x8F92EAB1
// (zstd seekable format, contrib/seekable_format/zstd_seekable_compression_format.md; little endian.  Descriptor 0: entries of 8 bytes, no per-frame
// checksums; with content checksums (`hash` != null) descriptor 0x80 = Checksum_Flag and entries of 12 bytes, the third word the low 32 bits of XXH64 of
// the frame's content -- the value the frame itself ends with)
extern "C" __global__ void __launch_bounds__(FRAME_T)
gc_zstd_emit_kernel(const uint8_t* __restrict__ src, uint64_t srcSize, const uint8_t* __restrict__ litSec,
                    const uint8_t* __restrict__ seqSec, const GcSectionInfo* __restrict__ info,
                    const GcFramePlan* __restrict__ plan, const uint64_t* __restrict__ result, uint32_t nBlocks, uint32_t frameBlocks,
                    uint8_t* __restrict__ dst, const uint64_t* __restrict__ hash /* per frame, or null: no content checksums */)
{
    if (result[1]) return;                       // output buffer too small: write nothing
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    if (b == nBlocks) {                          // the seek table (only launched when one is wanted)
        const uint32_t nFrames = (nBlocks + frameBlocks - 1u) / frameBlocks;
        const uint64_t entry = hash ? 12ull : 8ull;
        const uint64_t tableBytes = 8ull + entry * nFrames + 9ull, framesEnd = result[0] - tableBytes;
        uint8_t* o = dst + framesEnd;
        auto put32 = [](uint8_t* q, uint32_t v) { q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8); q[2] = (uint8_t)(v >> 16); q[3] = (uint8_t)(v >> 24); };
        if (t == 0) { put32(o, 0x184D2A5Eu); put32(o + 4, (uint32_t)(tableBytes - 8ull)); }
        for (uint32_t f = t; f < nFrames; f += FRAME_T) {
            const uint32_t b0 = f * frameBlocks, b1 = b0 + frameBlocks;
            const uint64_t end = b1 < nBlocks ? plan[b1].off : framesEnd;
            put32(o + 8u + entry * f, (uint32_t)(end - plan[b0].off));
            put32(o + 12u + entry * f, frame_len_of(b0, frameBlocks, srcSize));
            if (hash) put32(o + 16u + entry * f, (uint32_t)hash[f]);
        }
        if (t == 0) { uint8_t* ft = o + 8u + entry * nFrames; put32(ft, nFrames); ft[4] = hash ? 0x80 : 0; put32(ft + 5, 0x8F92EAB1u); }
        return;
    }
    const uint64_t base = (uint64_t)b * GC_ZSTD_BLOCK_MAX;
    const uint32_t blockLen = (uint32_t)((srcSize - base) < GC_ZSTD_BLOCK_MAX ? (srcSize - base) : GC_ZSTD_BLOCK_MAX);
    const bool first = (b % frameBlocks) == 0u, last = (b % frameBlocks) == frameBlocks - 1u || b == nBlocks - 1u;
    frame_write_block(dst + plan[b].off, plan[b], info[b], first, last, frame_len_of(b, frameBlocks, srcSize), blockLen, src + base,
                      litSec + (uint64_t)b * GC_LITSEC_STRIDE, seqSec + (uint64_t)b * GC_SEQSEC_STRIDE, hash ? hash + b / frameBlocks : nullptr);
}

// ------------------------------------------------------------------------------------------------ batch forms (gc_zstd_batch.h)
// A batch runs in rounds of nRound items through the per-block workspace: block b of the workspace holds item b of `items` (the round's part of the item table), every
// item a frame of one block.  The output offset carries from round to round in result[0], the "too small" mark in result[1] stays once set; the host zeroes both
// in front of the first round.

// K4b: one workgroup; places the round's frames behind those of the rounds before and publishes { offset, size, raw } per item for the host to read back
extern "C" __global__ void __launch_bounds__(1024)
gc_zstd_plan_batch_kernel(const GcSectionInfo* __restrict__ info, const gc_batch_item* __restrict__ items, uint32_t nRound, uint64_t dstCap,
                          GcFramePlan* __restrict__ plan, gc_batch_result* __restrict__ results /* the round's part of the result table */,
                          uint64_t* __restrict__ result /* [0] bytes so far, [1] error */, uint32_t checksum)
{
    __shared__ uint32_t sWave[16];
    const uint32_t t = threadIdx.x;
    uint64_t carry = result[0];
    const uint64_t err = result[1];
    for (uint32_t tb = 0; tb < nRound; tb += 1024u) {
        const uint32_t b = tb + t;
        uint32_t size = 0, comp = 0;
        if (b < nRound) {
            const uint32_t blockLen = items[b].src_size;
            size = frame_block_size(info[b], blockLen, frame_hdr_size(blockLen), checksum ? 4u : 0u, comp);
        }
        uint32_t all;
        const uint32_t before = frame_excl_scan(size, sWave, &all);     // (its barriers also stand between every thread's read of result[] above and the write below)
        if (b < nRound) {
            GcFramePlan p; p.off = carry + before; p.size = size; p.compressed = comp; plan[b] = p;
            gc_batch_result r; r.dst_off = p.off; r.dst_size = size; r.flags = comp ? 0u : 1u; results[b] = r;
        }
        carry += all;
    }
    if (t == 0) { result[0] = carry; result[1] = (err || carry > dstCap) ? 1u : 0u; }
}

// K5b: one workgroup per item writes its frame; the raw-block fallback copies from the item's place in the input
extern "C" __global__ void __launch_bounds__(FRAME_T)
gc_zstd_emit_batch_kernel(const uint8_t* __restrict__ src, const gc_batch_item* __restrict__ items, const uint8_t* __restrict__ litSec,
                          const uint8_t* __restrict__ seqSec, const GcSectionInfo* __restrict__ info, const GcFramePlan* __restrict__ plan,
                          const uint64_t* __restrict__ result, uint8_t* __restrict__ dst, const uint64_t* __restrict__ hash /* per item of the round, or null */)
{
    if (result[1]) return;                       // output buffer too small: this round and the ones behind it write nothing
    const uint32_t b = blockIdx.x;
    const gc_batch_item it = items[b];
    frame_write_block(dst + plan[b].off, plan[b], info[b], true, true, it.src_size, it.src_size, src + it.src_off,
                      litSec + (uint64_t)b * GC_LITSEC_STRIDE, seqSec + (uint64_t)b * GC_SEQSEC_STRIDE, hash ? hash + b : nullptr);
}
