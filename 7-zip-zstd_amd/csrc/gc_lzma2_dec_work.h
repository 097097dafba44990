// gc_lzma2_dec_work.h -- the LZMA2 decoder's workspace, owned by a gc_ctx (gc_api.hip) and used by gc_lzma2_dec.h.  Include after the HIP runtime (or its emulator stand-in).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "gc_devbuf.h"
struct GcL2dWork {
    GcBuf<uint8_t> meta;                  // unit descriptors, their order, results, the two ticket counters
    uint32_t instance = 0;                // test hook (GC_L2D_INSTANCE): 1 / 2 = every unit through the lc + lp <= 3 / the lc + lp <= 4 kernel instance; 0 = by the unit's flags
    uint32_t nCU = 0;                     // compute units of the device (the launch's width)
    void* ev0 = nullptr; void* ev1 = nullptr; float ms = 0.f;       // HIP events around the kernels of the last call
};
// gc_lzma2_dec.h (compiled with gc_lzma2_frame.hip), called by the context's entry points (gc_api.hip)
void gc_l2d_release(GcL2dWork* w);
int gc_l2d_decode(hipStream_t st, GcL2dWork* w, const uint8_t* d_src, size_t n, const gc_lzma2_unit* units, size_t nUnits, uint8_t* d_dst, size_t dstCap, unsigned dictProp, size_t* produced, char* err, size_t errCap);
