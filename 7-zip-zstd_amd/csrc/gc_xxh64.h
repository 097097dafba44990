// gc_xxh64.h -- K0x: XXH64 of every zstd frame's content, for the frames' content checksums (a bare .zst ends every frame with the
// low 32 bits of XXH64 of its content, seed 0 -- ZSTD_writeEpilogue C/zstd/zstd_compress.c:5225-5232, switched on by CPP/7zip/Archive/ZstdHandler.cpp:276
// "checksumFlag = 1"; the hash itself: C/zstd/xxhash.h XXH64_update / XXH64_digest).
//
// XXH64 walks its input in stripes of 32 bytes, four 8-byte lanes x_0..x_3 per stripe, with one accumulator per lane:
//     acc_i = rotl(acc_i + x_i * P2, 31) * P1
// The four recurrences are serial in the stripe number, so a frame cannot be split: the parallelism is across frames (one workgroup each) and,
// inside a frame, in everything that is NOT on the chain.  Per tile of GC_XXH64_TILE bytes
//   waves 1..4  stage    coalesced 8-byte loads of the NEXT tile straight from the call's input, the products x * P2 into LDS (double buffered)
//   wave 0      chain    lanes 0..3 = the four accumulators: ds_read_b64 of a product, add, rotate, one 64-bit multiply by P1 per stripe
// so the chain never waits for HBM and half of the 64-bit multiplies leave it.  (The decoder's verify loop, gc_zstd_dec.hip, lets the four lanes load
// their own 8 bytes per step from global memory: fine where the content has just been written and is verified once, the wrong shape for the encode path.)
// Behind the last whole stripe thread 0 runs XXH64's finalisation over the <= 31 bytes left.  One uint64 per frame goes to the workspace; K4 / K5
// (gc_zstd_frame.hip, which includes this file: the kernel is compiled beside them) put its low 32 bits behind the frame's last block and into the seek table.
#pragma once
#include "gc_common.h"
#include "gc_device.h"
#include "gpucodec.h"      // gc_batch_item

#define XXH_T        GC_XXH64_T                    // wave 0 chains, waves 1..4 stage
#define XXH_STAGERS  (XXH_T - 64u)
#define XXH_TILE     GC_XXH64_TILE                 // bytes per staged tile (gc_common.h; a multiple of the 32-byte stripe)
#define XXH_WORDS    (XXH_TILE / 8u)
#define XXH_PER      (XXH_WORDS / XXH_STAGERS)     // 8-byte words per stager and tile: all loads of a tile are in flight together
static_assert(XXH_WORDS % XXH_STAGERS == 0u && XXH_TILE % 32u == 0u, "tile geometry");

#define XXP1 0x9E3779B185EBCA87ull
#define XXP2 0xC2B2AE3D27D4EB4Full
#define XXP3 0x165667B19E3779F9ull
#define XXP4 0x85EBCA77C2B2AE63ull
#define XXP5 0x27D4EB2F165667C5ull

__device__ __forceinline__ uint64_t xx_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
__device__ __forceinline__ uint64_t xx_round(uint64_t acc, uint64_t x) { return xx_rotl(acc + x * XXP2, 31) * XXP1; }

// products of the whole stripes of tile `tile` (bytes [tile * XXH_TILE, min(+ XXH_TILE, stripeBytes)) of the frame) into `prod`; s = 0 .. XXH_STAGERS - 1
__device__ __forceinline__ void xx_stage(const uint8_t* __restrict__ p, uint64_t tile, uint64_t stripeBytes, uint64_t* prod, uint32_t s)
{
    const uint64_t base = tile * XXH_TILE;
    const uint32_t words = (uint32_t)((stripeBytes - base) < XXH_TILE ? (stripeBytes - base) : XXH_TILE) >> 3;
    if (words == XXH_WORDS) {                                  // a whole tile: every load is issued before the first product is needed
        uint64_t x[XXH_PER];
#pragma unroll
        for (uint32_t j = 0; j < XXH_PER; j++) x[j] = gc_ld64(p + base + 8ull * (s + j * XXH_STAGERS));
#pragma unroll
        for (uint32_t j = 0; j < XXH_PER; j++) prod[s + j * XXH_STAGERS] = x[j] * XXP2;
    } else                                                     // the frame's last tile
        for (uint32_t w = s; w < words; w += XXH_STAGERS) prod[w] = gc_ld64(p + base + 8ull * w) * XXP2;
}

struct XxLds { uint64_t prod[2][XXH_WORDS]; uint64_t acc[4]; };      // the calling kernel's LDS: staged products (double buffered), the four accumulators

// out[0] = XXH64(len bytes at p, seed), by the whole workgroup
__device__ __forceinline__ void xx_frame(const uint8_t* __restrict__ const p, const uint64_t len, const uint64_t seed, uint64_t* __restrict__ out, XxLds& L)
{
    uint64_t (&sProd)[2][XXH_WORDS] = L.prod;
    uint64_t (&sAcc)[4] = L.acc;
    const uint32_t t = threadIdx.x;
    const uint64_t stripeBytes = len & ~31ull;
    const uint64_t nTiles = (stripeBytes + XXH_TILE - 1u) / XXH_TILE;
    uint64_t acc = seed + (t == 0u ? XXP1 + XXP2 : (t == 1u ? XXP2 : (t == 2u ? 0ull : 0ull - XXP1)));
    if (t >= 64u && nTiles) xx_stage(p, 0, stripeBytes, sProd[0], t - 64u);
    __syncthreads();
    for (uint64_t k = 0; k < nTiles; k++) {
        if (t >= 64u) {
            if (k + 1u < nTiles) xx_stage(p, k + 1u, stripeBytes, sProd[(k + 1u) & 1u], t - 64u);
        } else if (t < 4u) {
            const uint64_t base = k * XXH_TILE;
            const uint32_t steps = (uint32_t)((stripeBytes - base) < XXH_TILE ? (stripeBytes - base) : XXH_TILE) >> 5;
            const uint64_t* const q = sProd[k & 1u] + t;
#pragma unroll 16
            for (uint32_t i = 0; i < steps; i++) acc = xx_rotl(acc + q[4u * i], 31) * XXP1;
        }
        __syncthreads();
    }
    if (t < 4u) sAcc[t] = acc;
    __syncthreads();
    if (t == 0u) {
        uint64_t h;
        if (len >= 32u) {
            h = xx_rotl(sAcc[0], 1) + xx_rotl(sAcc[1], 7) + xx_rotl(sAcc[2], 12) + xx_rotl(sAcc[3], 18);
            for (int k = 0; k < 4; k++) h = (h ^ xx_round(0, sAcc[k])) * XXP1 + XXP4;
        } else h = seed + XXP5;
        h += len;
        uint64_t pos = stripeBytes;
        while (pos + 8u <= len) { h ^= xx_round(0, gc_ld64(p + pos)); h = xx_rotl(h, 27) * XXP1 + XXP4; pos += 8u; }
        if (pos + 4u <= len) { h ^= (uint64_t)gc_ld32(p + pos) * XXP1; h = xx_rotl(h, 23) * XXP2 + XXP3; pos += 4u; }
        while (pos < len) { h ^= (uint64_t)p[pos] * XXP5; h = xx_rotl(h, 11) * XXP1; pos++; }
        h ^= h >> 33; h *= XXP2; h ^= h >> 29; h *= XXP3; h ^= h >> 32;
        out[0] = h;
    }
}

// frame f = bytes [f * frameBytes, min(srcSize, (f + 1) * frameBytes)) of src; out[f] = XXH64(frame, seed)
extern "C" __global__ void __launch_bounds__(XXH_T)
gc_zstd_xxh64_kernel(const uint8_t* __restrict__ src, uint64_t srcSize, uint64_t frameBytes, uint32_t nFrames, uint64_t seed, uint64_t* __restrict__ out)
{
    __shared__ XxLds L;
    const uint32_t f = blockIdx.x;
    if (f >= nFrames) return;
    const uint64_t start = (uint64_t)f * frameBytes;
    xx_frame(src + start, (srcSize - start) < frameBytes ? (srcSize - start) : frameBytes, seed, out + f, L);
}

// K0x of a batch (gc_zstd_batch.h): frame f = item f of the table, seed 0
extern "C" __global__ void __launch_bounds__(XXH_T)
gc_zstd_xxh64_batch_kernel(const uint8_t* __restrict__ src, const gc_batch_item* __restrict__ items, uint64_t* __restrict__ out)
{
    __shared__ XxLds L;
    const gc_batch_item it = items[blockIdx.x];
    xx_frame(src + it.src_off, it.src_size, 0, out + blockIdx.x, L);
}
