// gc_devbuf.h -- the one type that owns device memory of a context (gc_ctx, GcBrDecWork, GcL2dWork) and the one rule by which it grows.
// Include after the HIP runtime (or its emulator stand-in).
#pragma once
#include <stddef.h>
#include "gpucodec.h"

// A device allocation and the bytes of it that count: a member frees itself with its owner, so a new buffer is one member and one gc_buf_reserve call.
struct GcBufRaw {
    void* p = nullptr;
    size_t cap = 0;           // bytes a caller may ask for without another allocation (the padding of gc_buf_reserve is not in it)
    GcBufRaw() = default;
    GcBufRaw(const GcBufRaw&) = delete;
    GcBufRaw& operator=(const GcBufRaw&) = delete;
    ~GcBufRaw() { (void)hipFree(p); }
};
template <typename T> struct GcBuf : GcBufRaw { operator T*() const { return (T*)p; } };      // (kernel launches and pointer arithmetic take it as the T* it holds)

static inline void gc_buf_release(GcBufRaw& b) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }

// At least `need` bytes in b; what b holds is NOT carried over.  A growth allocates need + slack + pad bytes and records need + slack: the slack is room for the next calls, the
// padding lets a kernel read a few bytes past the end.  The new buffer is allocated while the old one still exists (a growth that fits needs no second try); if that fails
// the old one is freed and the allocation tried once more.  A failed growth leaves b empty (null, capacity 0) and returns GC_ERR_NOMEM -- the caller words the message.
// fill >= 0: the fresh buffer starts filled with that byte, on stream st (test hook GC_POISON_WORKSPACE of gc_api.hip).
static inline int gc_buf_reserve(GcBufRaw& b, size_t need, size_t pad = 0, size_t slack = 0, int fill = -1, hipStream_t st = nullptr)
{
    if (need <= b.cap) return GC_OK;
    const size_t cap = need + slack;
    void* np = nullptr;
    if (hipMalloc(&np, cap + pad) != hipSuccess) {
        gc_buf_release(b);
        if (hipMalloc(&np, cap + pad) != hipSuccess) return GC_ERR_NOMEM;
    }
    (void)hipFree(b.p); b.p = np; b.cap = cap;
    if (fill >= 0 && hipMemsetAsync(np, fill, cap + pad, st) != hipSuccess) return GC_ERR_HIP;
    return GC_OK;
}
