// gc_crc_seg.h -- the checks of MANY segments of one device buffer in one launch: CRC-64/XZ (C/XzCrc64.c: reflected polynomial 0xC96C5795D7870F42, initial value and final XOR
// all ones) and CRC-32 (the table and operators of gc_crc.hip) for the blocks of an .xz file, whose Check field is the CRC of the block's content (gc_xz.h).  Included at the end
// of gc_crc.hip: the kernels are compiled beside gc_crc32_chunk_kernel, which stays as it is.
//
// The structure is gc_crc.hip's -- one lane per 4 KiB slice through a byte table in LDS, the 256 slices of a 1 MiB piece folded in LDS with the eight fixed operators
// x^(8 * 4096 * 2^k), the pieces of a segment and the initial value's own shift folded on the host -- with one difference: a segment is cut into pieces from its END.
// R(M), the register after M starting from 0, does not change when zero bytes are put IN FRONT of M, so a short piece (the first of its segment) counts as a whole one whose
// leading slices are empty (R = 0) and whose first non-empty slice is short; every slice and every piece behind it is a whole one, the fixed operators are all the kernel
// needs, and no tail goes to the host byte by byte: a file of thousands of blocks costs one launch and one copy of 8 bytes per piece.  Segments start at any byte: a slice is
// read with unaligned 8-byte loads (gc_ld64, as gc_xxh64.h reads its frames), the up to seven bytes in front of them one by one.
#pragma once

struct GcCrc64Ops { uint64_t table[256]; uint64_t shift[8][64]; };      // shift[k][i] = image of bit i under "append 4096 * 2^k zero bytes"
struct GcCrcPiece { uint64_t start; uint32_t len; uint32_t seg; };      // bytes [start, start + len) of the buffer, 1 <= len <= CRC_CHUNK, ending where a piece of segment `seg` ends

template <typename R, uint32_t BITS> __device__ __forceinline__ R crcseg_apply(const R* m, R v)
{
    R r = 0;
#pragma unroll
    for (uint32_t i = 0; i < BITS; i++) r ^= ((v >> i) & 1u) ? m[i] : (R)0;
    return r;
}

// out[p] = R(piece p); one workgroup of CRC_T lanes per piece
template <typename R, uint32_t BITS, typename OPS>
__device__ __forceinline__ void crcseg_body(const uint8_t* __restrict__ src, const GcCrcPiece* __restrict__ pieces, uint32_t nPieces, const OPS* __restrict__ ops, R* __restrict__ out)
{
    __shared__ R sTab[256];
    __shared__ R sShift[8][BITS];
    __shared__ R sR[CRC_T];
    const uint32_t t = threadIdx.x, c = blockIdx.x;
    if (c >= nPieces) return;
    sTab[t] = ops->table[t];
    for (uint32_t i = t; i < 8u * BITS; i += CRC_T) sShift[i / BITS][i % BITS] = ops->shift[i / BITS][i % BITS];
    __syncthreads();
    const GcCrcPiece pc = pieces[c];
    // slice t ends (CRC_T - 1 - t) slices in front of the piece's end; what lies in front of the piece's first byte is not read
    const int64_t relEnd = (int64_t)pc.len - (int64_t)(CRC_T - 1u - t) * (int64_t)CRC_SLICE;
    R r = 0;
    if (relEnd > 0) {
        const uint32_t relStart = relEnd > (int64_t)CRC_SLICE ? (uint32_t)relEnd - CRC_SLICE : 0u;
        const uint32_t m = (uint32_t)relEnd - relStart;                       // 1 .. CRC_SLICE bytes
        const uint8_t* p = src + pc.start + relStart;
        for (uint32_t i = 0; i < (m & 7u); i++) r = sTab[(uint32_t)(r ^ *p++) & 0xFFu] ^ (r >> 8);
        const uint32_t words = m >> 3;
        uint64_t nxt = words ? gc_ld64(p) : 0ull;
        for (uint32_t i = 0; i < words; i++) {
            const uint64_t w = nxt;
            if (i + 1u < words) nxt = gc_ld64(p + 8u * (i + 1u));
            if (BITS == 64u) {
                r ^= (R)w;                                                    // eight bytes at a time through the byte table
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) r = sTab[(uint32_t)r & 0xFFu] ^ (r >> 8);
            } else {
#pragma unroll
                for (uint32_t h = 0; h < 2u; h++) {
                    r ^= (R)(w >> (32u * h));
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) r = sTab[(uint32_t)r & 0xFFu] ^ (r >> 8);
                }
            }
        }
    }
    sR[t] = r;
    __syncthreads();
    for (uint32_t k = 0; k < 8u; k++) {                           // fold pairs: left value shifted over the right one's 4096 * 2^k bytes
        const uint32_t stride = 1u << k;
        R v = 0;
        const bool on = (t & (2u * stride - 1u)) == 0u;
        if (on) v = crcseg_apply<R, BITS>(sShift[k], sR[t]) ^ sR[t + stride];
        __syncthreads();
        if (on) sR[t] = v;
        __syncthreads();
    }
    if (t == 0) out[c] = sR[0];
}

extern "C" __global__ void __launch_bounds__(CRC_T)
gc_crc64_seg_kernel(const uint8_t* __restrict__ src, const GcCrcPiece* __restrict__ pieces, uint32_t nPieces, const GcCrc64Ops* __restrict__ ops, uint64_t* __restrict__ out)
{
    crcseg_body<uint64_t, 64u, GcCrc64Ops>(src, pieces, nPieces, ops, out);
}
extern "C" __global__ void __launch_bounds__(CRC_T)
gc_crc32_seg_kernel(const uint8_t* __restrict__ src, const GcCrcPiece* __restrict__ pieces, uint32_t nPieces, const GcCrcOps* __restrict__ ops, uint32_t* __restrict__ out)
{
    crcseg_body<uint32_t, 32u, GcCrcOps>(src, pieces, nPieces, ops, out);
}

// ---------------------------------------------------------------------------------------------------- host side
// The register as a polynomial over GF(2), reflected: bit BITS-1 is x^0.  "Append one zero bit" is the multiplication by x modulo the polynomial, so appending n zero bytes
// is the multiplication by x^(8 n): one square-and-multiply per segment length instead of a matrix product per bit of it.
template <typename R> struct CrcSegField {
    R poly, one;
    R mulx(R a) const { return (R)((a >> 1) ^ (poly & ((R)0 - (a & (R)1)))); }
    R mul(R a, R b) const { R r = 0; for (R bit = one; bit; bit >>= 1) { if (b & bit) r ^= a; a = mulx(a); } return r; }
    R xpow8(uint64_t nBytes) const       // x^(8 nBytes)
    {
        R acc = one, sq = mulx(one);      // x^0, x^1
        for (int i = 0; i < 3; i++) sq = mul(sq, sq);                         // x^8
        for (; nBytes; nBytes >>= 1) { if (nBytes & 1u) acc = mul(acc, sq); sq = mul(sq, sq); }
        return acc;
    }
};
static uint64_t crc64_byte_table_entry(uint32_t i) { uint64_t r = i; for (int k = 0; k < 8; k++) r = (r >> 1) ^ (0xC96C5795D7870F42ull & (0ull - (r & 1u))); return r; }

// kind: the check id of the xz format, GC_XZ_CHECK_CRC32 (1) or GC_XZ_CHECK_CRC64 (4).  out[i] = the check of bytes [segs[i].offset, + segs[i].length) of d_src; host memory.
// On the calling thread's stream (gc_host_stream.h), with scratch from there; synchronous.  evStart / evEnd (may be null): recorded around the launch.
// *launches (may be null) counts the kernel launches: 1, or 0 when every segment is empty.
int gc_crc_segments_run(int kind, const void* d_src, const gc_crc_segment* segs, size_t nSegs, uint64_t* out, hipEvent_t evStart, hipEvent_t evEnd, unsigned* launches)
{
    if (launches) *launches = 0;
    if ((kind != 1 && kind != 4) || (!segs && nSegs) || (!out && nSegs)) return GC_ERR_PARAM;
    const bool wide = kind == 4;
    static GcCrc64Ops ops64; static GcCrcOps ops32; static bool built = false;
    static const CrcSegField<uint64_t> F64 = { 0xC96C5795D7870F42ull, 1ull << 63 };
    static const CrcSegField<uint32_t> F32 = { 0xEDB88320u, 1u << 31 };
    if (!built) {
        for (uint32_t i = 0; i < 256u; i++) { ops64.table[i] = crc64_byte_table_entry(i); ops32.table[i] = crc_byte_table_entry(i); }
        for (uint32_t k = 0; k < 8u; k++) {
            const uint64_t s64 = F64.xpow8((uint64_t)CRC_SLICE << k);
            for (uint32_t i = 0; i < 64u; i++) ops64.shift[k][i] = F64.mul(1ull << i, s64);
            crc_shift_op(ops32.shift[k], (uint64_t)CRC_SLICE << k);
        }
        built = true;
    }
    size_t nPieces = 0;
    for (size_t i = 0; i < nSegs; i++) {
        if (segs[i].length && !d_src) return GC_ERR_PARAM;
        if (segs[i].offset + segs[i].length < segs[i].offset) return GC_ERR_PARAM;
        nPieces += (size_t)((segs[i].length + CRC_CHUNK - 1u) / CRC_CHUNK);
    }
    if (nPieces > 0x7FFFFFFFu || nSegs > 0xFFFFFFFFu) return GC_ERR_PARAM;
    uint64_t* hOut = nullptr; GcCrcPiece* hp = nullptr;
    if (nPieces) {
        hp = (GcCrcPiece*)malloc(nPieces * sizeof(GcCrcPiece)); hOut = (uint64_t*)malloc(nPieces * sizeof(uint64_t));
        if (!hp || !hOut) { free(hp); free(hOut); return GC_ERR_NOMEM; }
        size_t k = 0;
        for (size_t i = 0; i < nSegs; i++) {
            const uint64_t len = segs[i].length, cnt = (len + CRC_CHUNK - 1u) / CRC_CHUNK;
            for (uint64_t j = 0; j < cnt; j++) {                                  // piece j ends (cnt - 1 - j) whole pieces in front of the segment's end: the first one is the short one
                const uint64_t end = len - (cnt - 1u - j) * CRC_CHUNK, beg = end > CRC_CHUNK ? end - CRC_CHUNK : 0u;
                hp[k].start = segs[i].offset + beg; hp[k].len = (uint32_t)(end - beg); hp[k].seg = (uint32_t)i; k++;
            }
        }
        // one scratch buffer: operators, pieces, results
        const size_t opsBytes = wide ? sizeof(GcCrc64Ops) : sizeof(GcCrcOps), oPieces = (opsBytes + 63u) & ~(size_t)63u, oOut = oPieces + ((nPieces * sizeof(GcCrcPiece) + 63u) & ~(size_t)63u);
        uint8_t* d = nullptr;
        if (gc_scratch_alloc((void**)&d, oOut + nPieces * sizeof(uint64_t)) != hipSuccess) { free(hp); free(hOut); return GC_ERR_NOMEM; }
        bool ok = hipMemcpyAsync(d, wide ? (const void*)&ops64 : (const void*)&ops32, opsBytes, hipMemcpyHostToDevice, gc_tls_stream) == hipSuccess
               && hipMemcpyAsync(d + oPieces, hp, nPieces * sizeof(GcCrcPiece), hipMemcpyHostToDevice, gc_tls_stream) == hipSuccess;
        if (ok) {
            if (evStart) hipEventRecord(evStart, gc_tls_stream);
            if (wide) GC_LAUNCH(gc_crc64_seg_kernel, (uint32_t)nPieces, CRC_T, gc_tls_stream, (const uint8_t*)d_src, (const GcCrcPiece*)(d + oPieces), (uint32_t)nPieces, (const GcCrc64Ops*)d, (uint64_t*)(d + oOut));
            else GC_LAUNCH(gc_crc32_seg_kernel, (uint32_t)nPieces, CRC_T, gc_tls_stream, (const uint8_t*)d_src, (const GcCrcPiece*)(d + oPieces), (uint32_t)nPieces, (const GcCrcOps*)d, (uint32_t*)(d + oOut));
            if (evEnd) hipEventRecord(evEnd, gc_tls_stream);
            if (launches) *launches = 1;
            ok = hipGetLastError() == hipSuccess;
        }
        ok = gc_copy_sync(hOut, d + oOut, nPieces * (wide ? 8u : 4u), hipMemcpyDeviceToHost) == hipSuccess && ok;      // (waits for the stream whatever happened: the host arrays are free afterwards)
        gc_scratch_free(d);
        if (!ok) { free(hp); free(hOut); return GC_ERR_HIP; }
    } else if (evStart && evEnd) { hipEventRecord(evStart, gc_tls_stream); hipEventRecord(evEnd, gc_tls_stream); }
    // per segment: the pieces (all but the first are whole: one fixed multiplication each), the initial value's shift over the whole length, the final XOR
    const uint64_t c64 = F64.xpow8(CRC_CHUNK); const uint32_t c32 = F32.xpow8(CRC_CHUNK);
    size_t k = 0;
    for (size_t i = 0; i < nSegs; i++) {
        const uint64_t len = segs[i].length, cnt = (len + CRC_CHUNK - 1u) / CRC_CHUNK;
        if (wide) {
            uint64_t reg = 0;
            for (uint64_t j = 0; j < cnt; j++) reg = F64.mul(reg, c64) ^ hOut[k++];
            out[i] = reg ^ F64.mul(~0ull, F64.xpow8(len)) ^ ~0ull;
        } else {
            uint32_t reg = 0;
            for (uint64_t j = 0; j < cnt; j++) reg = F32.mul(reg, c32) ^ ((const uint32_t*)hOut)[k++];
            out[i] = (uint32_t)(reg ^ F32.mul(0xFFFFFFFFu, F32.xpow8(len)) ^ 0xFFFFFFFFu);
        }
    }
    free(hp); free(hOut);
    return GC_OK;
}

// CRC-64/XZ of n bytes in device memory ("123456789" -> 0x995DC9BBDF1939FA): one segment through the launch above.  On the calling thread's stream, synchronous like gc_crc32_device.
extern "C" int gc_crc64_device(const void* d_src, size_t n, uint64_t* crc)
{
    if ((!d_src && n) || !crc) return GC_ERR_PARAM;
    const gc_crc_segment seg = { 0u, (uint64_t)n };
    return gc_crc_segments_run(4, d_src, &seg, 1, crc, nullptr, nullptr, nullptr);
}
