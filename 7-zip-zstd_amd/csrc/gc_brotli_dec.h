// gc_brotli_dec.h -- the BROTLI decoder's workspace, owned by a gc_ctx (gc_api.hip) and used by gc_brotli_dec.hip.  Include after the HIP runtime (or its emulator stand-in).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "gc_devbuf.h"
struct GcBrDecWork {
    GcBuf<uint8_t> stage;                 // every chunk decodes into a slot of its hint size
    GcBuf<uint8_t> pages;                 // HBM behind the LDS arenas (meta-blocks with hundreds of prefix codes): whole pages of BRD_PAGE bytes
    GcBuf<uint8_t> meta;                  // chunk descriptors, results, offsets, totals, the page cursor
    GcBuf<uint8_t> dict; uint64_t dictStamp = 0;      // the static dictionary on this device, if the process holds one
    uint32_t instance = 0;                // test hook (GC_BRD_INSTANCE): 1-4 = the kernel instance (LDS arena / ring size) whatever the number of chunks; 0 = by the number of chunks
    uint32_t ldsCap = 0;                  // test hook (GC_BRD_LDS): a smaller LDS arena, so that small inputs take the HBM pages; 0 = the kernel's own
    void* ev0 = nullptr; void* ev1 = nullptr; float ms = 0.f;       // HIP events around the kernels of the last call
};
// gc_brotli_dec.hip, called by the context's entry points (gc_api.hip)
void gc_brd_release(GcBrDecWork* w);
int gc_brd_decode(hipStream_t st, GcBrDecWork* w, const uint8_t* d_src, const gc_brotli_chunk* chunks, size_t nChunks, uint8_t* d_dst, size_t dstCap, size_t* produced, char* err, size_t errCap);
