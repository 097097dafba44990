// gc_xz.h -- the .xz container around LZMA2 (the third format the reference reads and writes bare -- C/Xz.c, XzEnc.c, XzDec.c, XzIn.c -- after .zst and .br),
// written from "The .xz File Format" 1.0.4.  Included at the end of gc_api.hip: host code over the context, the FLZMA2 encoder, the LZMA2 decoder (gc_lzma2_dec.h) and the
// segmented CRC kernels (gc_crc_seg.h), and one small kernel that collects the stored Checks of a file that lies in device memory.
//
//   Stream        = Stream Header (12) | Block ... | Index | Stream Footer (12)          several streams may follow each other, zero bytes in a multiple of four between / behind them
//   Stream Header = FD 37 7A 58 5A 00 | flags: 00, check id | CRC-32 of the flags
//   Block         = Block Header | LZMA2 stream | 0..3 zero bytes up to a multiple of four | Check (0, 4 or 8 bytes: none, CRC-32, CRC-64 of the content, little endian)
//   Block Header  = size / 4 - 1 | flags (bits 0-1 filters - 1, bit 6 / 7: packed / unpacked size present) | [packed] [unpacked] | filters: id, size of properties, properties |
//                   zero bytes up to the stated size | CRC-32 of all of that
//   Index         = 00 | number of records | per Block: unpadded size (header + payload + check), unpacked size | 0..3 zero bytes | CRC-32 of all of that
//   Stream Footer = CRC-32 of the next six bytes | Index size / 4 - 1 | flags as in the header | 59 5A
// Sizes and counts are "multibyte integers": seven bits per byte from the low end, bit 7 = another byte follows, nine bytes at most, no zero byte at the end of a longer one.
//
// What makes the container worth having on this engine: the Blocks are independent LZMA2 streams and the Index says where each one lies, so the decoder hands the units of ALL
// Blocks to one gc_l2d_decode call (one wave per unit, side by side) and checks all contents with one launch of the segmented CRC kernel; the encoder cuts its input into
// Blocks, so its own files decode that way, and takes all Checks from one launch over the input where it lies in HBM.
#pragma once
#include <vector>

int gc_crc_segments_run(int kind, const void* d_src, const gc_crc_segment* segs, size_t nSegs, uint64_t* out, hipEvent_t evStart, hipEvent_t evEnd, unsigned* launches);      // (gc_crc_seg.h)

// ------------------------------------------------------------------------------------------------ the format's small parts
static uint32_t xz_crc32(const uint8_t* p, size_t n)      // the headers' CRC-32 (a few bytes each: computed where they are written or read, on the host)
{
    static uint32_t tab[256]; static bool built = false;
    if (!built) { for (uint32_t i = 0; i < 256u; i++) { uint32_t r = i; for (int k = 0; k < 8; k++) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u))); tab[i] = r; } built = true; }
    uint32_t r = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) r = tab[(r ^ p[i]) & 0xFFu] ^ (r >> 8);
    return r ^ 0xFFFFFFFFu;
}
static uint32_t xz_le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void xz_put32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static size_t xz_vli_len(uint64_t v) { size_t k = 1; while (v >>= 7) k++; return k; }
static size_t xz_put_vli(uint8_t* p, uint64_t v) { size_t k = 0; while (v >= 0x80u) { p[k++] = (uint8_t)(v | 0x80u); v >>= 7; } p[k++] = (uint8_t)v; return k; }
// a multibyte integer at p[q .. end); false: it runs into `end`, is longer than nine bytes or ends in a zero byte
static bool xz_get_vli(const uint8_t* p, size_t& q, size_t end, uint64_t& v)
{
    v = 0;
    for (uint32_t i = 0; i < 9u; i++) {
        if (q >= end) return false;
        const uint8_t b = p[q++];
        if (b == 0u && i > 0u) return false;
        v |= (uint64_t)(b & 0x7Fu) << (7u * i);
        if (!(b & 0x80u)) return true;
    }
    return false;
}
static uint32_t xz_check_size(uint32_t id) { return id == GC_XZ_CHECK_NONE ? 0u : (id == GC_XZ_CHECK_CRC32 ? 4u : 8u); }      // (of the three this code handles)
static const uint8_t kXzMagic[6] = { 0xFD, 0x37, 0x7A, 0x58, 0x5A, 0x00 };
#define XZ_HEADER_MAX 32u      // a Block Header as the writer makes it: 2 + 9 + 9 + 3 bytes, padded, + 4

// ------------------------------------------------------------------------------------------------ reader
struct XzStreamSpan { size_t start, indexOff; uint32_t check; std::vector<uint64_t> recs; };      // recs: unpadded size, unpacked size per Block

// One stream, found from its end at `pos` (behind its footer): footer -> Index -> header.  GC_OK and the span, or the error.
static int xz_stream_backward(const uint8_t* p, size_t pos, XzStreamSpan& s)
{
    if (pos < 32u) return GC_ERR_CORRUPT;                                     // (header, empty Index and footer take 32 bytes)
    const uint8_t* f = p + pos - 12u;
    if (f[10] != 0x59u || f[11] != 0x5Au || xz_le32(f) != xz_crc32(f + 4, 6)) return GC_ERR_CORRUPT;
    const uint64_t indexSize = ((uint64_t)xz_le32(f + 4) + 1u) * 4u;
    if (indexSize > pos - 24u) return GC_ERR_CORRUPT;
    const size_t indexEnd = pos - 12u, indexOff = indexEnd - (size_t)indexSize;
    if (p[indexOff] != 0u || xz_le32(p + indexEnd - 4u) != xz_crc32(p + indexOff, (size_t)indexSize - 4u)) return GC_ERR_CORRUPT;
    size_t q = indexOff + 1u; const size_t qEnd = indexEnd - 4u;
    uint64_t count = 0;
    if (!xz_get_vli(p, q, qEnd, count) || count > indexSize / 2u) return GC_ERR_CORRUPT;
    s.recs.clear(); s.recs.reserve((size_t)count * 2u);
    uint64_t blocksBytes = 0;
    for (uint64_t i = 0; i < count; i++) {
        uint64_t unpadded = 0, unpacked = 0;
        if (!xz_get_vli(p, q, qEnd, unpadded) || !xz_get_vli(p, q, qEnd, unpacked)) return GC_ERR_CORRUPT;
        if (unpadded < 5u || unpadded > (uint64_t)indexOff) return GC_ERR_CORRUPT;
        blocksBytes += (unpadded + 3u) & ~3ull;
        if (blocksBytes > (uint64_t)indexOff) return GC_ERR_CORRUPT;
        s.recs.push_back(unpadded); s.recs.push_back(unpacked);
    }
    if (qEnd - q > 3u) return GC_ERR_CORRUPT;                                 // Index Padding: up to the next multiple of four, zero bytes
    for (; q < qEnd; q++) if (p[q] != 0u) return GC_ERR_CORRUPT;
    if ((uint64_t)indexOff < blocksBytes + 12u) return GC_ERR_CORRUPT;
    const size_t start = indexOff - (size_t)blocksBytes - 12u;
    const uint8_t* h = p + start;
    if (memcmp(h, kXzMagic, 6) != 0 || xz_le32(h + 8) != xz_crc32(h + 6, 2)) return GC_ERR_CORRUPT;
    if (h[6] != f[8] || h[7] != f[9]) return GC_ERR_CORRUPT;                  // the footer's flags are the header's
    if (h[6] != 0u || (h[7] & 0xF0u)) return GC_ERR_UNSUPPORTED;              // reserved bits: a later version of the format
    s.check = h[7] & 0x0Fu;
    if (s.check != GC_XZ_CHECK_NONE && s.check != GC_XZ_CHECK_CRC32 && s.check != GC_XZ_CHECK_CRC64) return GC_ERR_UNSUPPORTED;      // SHA-256 (10) and the ids without a definition
    s.start = start; s.indexOff = indexOff;
    return GC_OK;
}

// The Block at p[off ...] whose Index record says (unpadded, unpacked), in a stream with check `check`: the header's own CRC, its filter chain, its sizes against the record's,
// the padding behind the payload.  Fills src_off / src_size / dst_size / check_off / check / dict_prop.
static int xz_block_header(const uint8_t* p, size_t off, uint64_t unpadded, uint64_t unpacked, uint32_t check, gc_xz_block& b)
{
    const uint32_t hs = p[off];                                               // (unpadded >= 5: the first bytes of the header lie inside the Block)
    if (hs == 0u) return GC_ERR_CORRUPT;                                      // (0 is the Index Indicator)
    const uint64_t hdrSize = ((uint64_t)hs + 1u) * 4u, checkSize = xz_check_size(check);
    if (hdrSize + checkSize >= unpadded) return GC_ERR_CORRUPT;               // no room for a payload
    if (xz_le32(p + off + hdrSize - 4u) != xz_crc32(p + off, (size_t)hdrSize - 4u)) return GC_ERR_CORRUPT;
    const uint32_t flags = p[off + 1u];
    if (flags & 0x3Cu) return GC_ERR_UNSUPPORTED;                             // reserved bits
    size_t q = off + 2u; const size_t qEnd = off + (size_t)hdrSize - 4u;
    const uint64_t packed = unpadded - hdrSize - checkSize;
    uint64_t v = 0;
    if ((flags & 0x40u) && (!xz_get_vli(p, q, qEnd, v) || v != packed)) return GC_ERR_CORRUPT;
    if ((flags & 0x80u) && (!xz_get_vli(p, q, qEnd, v) || v != unpacked)) return GC_ERR_CORRUPT;
    const uint32_t nFilters = (flags & 3u) + 1u;
    bool lzma2Alone = nFilters == 1u; uint32_t prop = 0;
    for (uint32_t i = 0; i < nFilters; i++) {
        uint64_t id = 0, propsSize = 0;
        if (!xz_get_vli(p, q, qEnd, id) || !xz_get_vli(p, q, qEnd, propsSize) || propsSize > (uint64_t)(qEnd - q)) return GC_ERR_CORRUPT;
        if (id != 0x21u) lzma2Alone = false;
        else if (propsSize != 1u) return GC_ERR_CORRUPT;
        else prop = p[q];
        q += (size_t)propsSize;
    }
    for (; q < qEnd; q++) if (p[q] != 0u) return GC_ERR_CORRUPT;              // Header Padding
    if (!lzma2Alone) return GC_ERR_UNSUPPORTED;                               // BCJ / Delta in front of LZMA2, or another coder: refused, never passed through
    if (prop > 40u) return GC_ERR_CORRUPT;
    const size_t payload = off + (size_t)hdrSize, padded = (size_t)((packed + 3u) & ~3ull);
    for (size_t i = (size_t)packed; i < padded; i++) if (p[payload + i] != 0u) return GC_ERR_CORRUPT;      // Block Padding
    b.src_off = payload; b.src_size = packed; b.dst_size = unpacked; b.check_off = payload + padded; b.check = check; b.dict_prop = prop;
    return GC_OK;
}

static int xz_scan(const uint8_t* p, size_t n, std::vector<gc_xz_block>& blocks, std::vector<gc_lzma2_unit>& units, uint64_t* contentTotal)
{
    std::vector<XzStreamSpan> streams;                                        // last stream first
    size_t pos = n;
    for (;;) {
        while (pos >= 4u && xz_le32(p + pos - 4u) == 0u) pos -= 4u;          // Stream Padding
        if (pos == 0u) return GC_ERR_CORRUPT;                                 // no stream at all, or zero bytes in front of the first one
        streams.emplace_back();
        const int rc = xz_stream_backward(p, pos, streams.back());
        if (rc != GC_OK) return rc;
        pos = streams.back().start;
        if (pos == 0u) break;
    }
    uint64_t dst = 0;
    for (size_t si = streams.size(); si-- > 0;) {
        const XzStreamSpan& s = streams[si];
        size_t off = s.start + 12u;
        for (size_t r = 0; r < s.recs.size(); r += 2u) {
            gc_xz_block b; memset(&b, 0, sizeof(b));
            int rc = xz_block_header(p, off, s.recs[r], s.recs[r + 1u], s.check, b);
            if (rc != GC_OK) return rc;
            size_t nu = 0, consumed = 0; int ended = 0; uint64_t total = 0;
            rc = gc_lzma2_scan_prefix(p + b.src_off, (size_t)b.src_size, nullptr, 0, &nu, &total, &consumed, &ended);
            if (rc != GC_OK) return GC_ERR_CORRUPT;
            if (!ended || consumed != b.src_size || total != b.dst_size) return GC_ERR_CORRUPT;      // whole units, the end marker, nothing behind it, the Index's size
            b.dst_off = dst; b.first_unit = (uint32_t)units.size(); b.n_units = (uint32_t)nu;
            if (units.size() + nu > 0xFFFFFFFFull) return GC_ERR_UNSUPPORTED;
            units.resize(units.size() + nu);
            if (nu) {
                rc = gc_lzma2_scan_prefix(p + b.src_off, (size_t)b.src_size, units.data() + b.first_unit, nu, &nu, &total, &consumed, &ended);
                if (rc != GC_OK) return GC_ERR_CORRUPT;
                for (size_t i = b.first_unit; i < units.size(); i++) { units[i].src_off += b.src_off; units[i].dst_off += dst; }
            }
            if (dst + b.dst_size < dst) return GC_ERR_CORRUPT;
            dst += b.dst_size;
            blocks.push_back(b);
            off = (size_t)b.check_off + xz_check_size(s.check);
        }
    }
    if (contentTotal) *contentTotal = dst;
    return GC_OK;
}

extern "C" int gc_xz_scan(const void* src, size_t n, gc_xz_block* blocks, size_t maxBlocks, size_t* nBlocks, gc_lzma2_unit* units, size_t maxUnits, size_t* nUnits, uint64_t* contentTotal)
{
    if ((!src && n) || !nBlocks) return GC_ERR_PARAM;
    *nBlocks = 0; if (nUnits) *nUnits = 0; if (contentTotal) *contentTotal = 0;
    if (!n) return GC_ERR_CORRUPT;
    std::vector<gc_xz_block> bl; std::vector<gc_lzma2_unit> un;
    const int rc = xz_scan((const uint8_t*)src, n, bl, un, contentTotal);
    if (rc != GC_OK) { if (contentTotal) *contentTotal = 0; return rc; }
    if ((blocks && bl.size() > maxBlocks) || (units && un.size() > maxUnits)) return GC_ERR_PARAM;
    if (blocks && !bl.empty()) memcpy(blocks, bl.data(), bl.size() * sizeof(gc_xz_block));
    if (units && !un.empty()) memcpy(units, un.data(), un.size() * sizeof(gc_lzma2_unit));
    *nBlocks = bl.size(); if (nUnits) *nUnits = un.size();
    return GC_OK;
}

// ------------------------------------------------------------------------------------------------ the checks of a call
// out[i] = the stored Check of block i (little endian, 0 / 4 / 8 bytes) of a file in device memory; words[i] = check_off << 4 | bytes
extern "C" __global__ void __launch_bounds__(256)
gc_xz_gather_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ words, uint32_t n, uint64_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t off = words[i] >> 4; const uint32_t bytes = (uint32_t)words[i] & 15u;
    uint64_t v = 0;
    for (uint32_t k = 0; k < bytes; k++) v |= (uint64_t)src[off + k] << (8u * k);
    out[i] = v;
}

static int xz_events(gc_ctx* c)
{
    for (int i = 0; i < 2; i++) if (!c->xzEv[i]) HIPCHK(c, hipEventCreate(&c->xzEv[i]));
    return GC_OK;
}

// the checks of `kind` over d_data for the listed segments, on the context's stream; adds the kernel's time and launch to the context's figures
static int xz_checks_run(gc_ctx* c, int kind, const void* d_data, const std::vector<gc_crc_segment>& segs, std::vector<uint64_t>& vals)
{
    vals.assign(segs.size(), 0u);
    if (segs.empty()) return GC_OK;
    const GcStreamScope onMine(c->stream);
    unsigned launches = 0;
    const int rc = gc_crc_segments_run(kind, d_data, segs.data(), segs.size(), vals.data(), c->xzEv[0], c->xzEv[1], &launches);
    if (rc != GC_OK) { snprintf(c->err, sizeof(c->err), "the check kernel failed over %zu segments", segs.size()); return rc; }
    if (launches) { float t = 0.f; HIPCHK(c, hipEventElapsedTime(&t, c->xzEv[0], c->xzEv[1])); c->xzMs[1] += t; c->xzCounts[2] += launches; }
    return GC_OK;
}

extern "C" int gc_crc_segments_device(gc_ctx* c, const void* d_src, const gc_crc_segment* segs, size_t nSegs, int check, uint64_t* out)
{
    if (!c || (check != GC_XZ_CHECK_CRC32 && check != GC_XZ_CHECK_CRC64) || (!segs && nSegs) || (!out && nSegs)) return GC_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    const GcStreamScope onMine(c->stream);
    return gc_crc_segments_run(check, d_src, segs, nSegs, out, nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------ decoder
// h_src: the file in host memory as well (the host entry point), or null: then the stored Checks are collected from d_src by gc_xz_gather_kernel
static int xz_decode(gc_ctx* c, const uint8_t* d_src, const uint8_t* h_src, size_t n, uint8_t* d_dst, size_t dstCap, const gc_xz_block* blocks, size_t nBlocks,
                     const gc_lzma2_unit* units, size_t nUnits, size_t* outSize)
{
    *outSize = 0;
    c->xzMs[0] = c->xzMs[1] = 0.f; c->xzCounts[0] = c->xzCounts[1] = c->xzCounts[2] = 0u;
    if (nBlocks > 0xFFFFFFFFu) return GC_ERR_PARAM;
    uint64_t total = 0; unsigned prop = 0; bool anyCheck = false;
    for (size_t i = 0; i < nBlocks; i++) {
        const gc_xz_block& b = blocks[i];
        if (b.check != GC_XZ_CHECK_NONE && b.check != GC_XZ_CHECK_CRC32 && b.check != GC_XZ_CHECK_CRC64) { snprintf(c->err, sizeof(c->err), "xz block %zu: check id %u is not handled", i, b.check); return GC_ERR_UNSUPPORTED; }
        if (b.dict_prop > 40u || b.check_off > n || xz_check_size(b.check) > n - b.check_off) { snprintf(c->err, sizeof(c->err), "xz block %zu: not a block of these %zu bytes", i, n); return GC_ERR_PARAM; }
        if (b.dst_off > dstCap || b.dst_size > dstCap - b.dst_off) { snprintf(c->err, sizeof(c->err), "destination too small: xz block %zu ends behind the %zu bytes of capacity", i, dstCap); return GC_ERR_DST_SMALL; }
        if (b.dict_prop > prop) prop = b.dict_prop;
        total += b.dst_size; anyCheck = anyCheck || b.check != GC_XZ_CHECK_NONE;
    }
    int rc = xz_events(c);
    if (rc != GC_OK) return rc;
    // every unit of every block in ONE decode call: the blocks run side by side
    size_t produced = 0;
    if (nUnits) {
        l2d_hooks(c);
        rc = gc_l2d_decode(c->stream, &c->l2d, d_src, n, units, nUnits, d_dst, dstCap, prop, &produced, c->err, sizeof(c->err));
        c->xzMs[0] = c->l2d.ms; c->xzCounts[0] = 1u; c->xzCounts[1] = (unsigned)nUnits;
        if (rc != GC_OK) return rc;
    }
    if (produced != total) { snprintf(c->err, sizeof(c->err), "the units hold %zu bytes, the xz blocks state %llu", produced, (unsigned long long)total); return GC_ERR_CORRUPT; }
    if (anyCheck) {
        // the stored values
        std::vector<uint64_t> stored(nBlocks, 0u);
        if (h_src) {
            for (size_t i = 0; i < nBlocks; i++) for (uint32_t k = 0; k < xz_check_size(blocks[i].check); k++) stored[i] |= (uint64_t)h_src[blocks[i].check_off + k] << (8u * k);
        } else {
            if (gc_buf_reserve(c->xzWork, 2u * nBlocks * sizeof(uint64_t)) != GC_OK) { snprintf(c->err, sizeof(c->err), "no device memory for the checks of %zu xz blocks", nBlocks); return GC_ERR_NOMEM; }
            std::vector<uint64_t> words(nBlocks);
            for (size_t i = 0; i < nBlocks; i++) words[i] = (blocks[i].check_off << 4) | xz_check_size(blocks[i].check);
            HIPCHK(c, hipMemcpyAsync(c->xzWork, words.data(), nBlocks * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
            GC_LAUNCH(gc_xz_gather_kernel, (uint32_t)((nBlocks + 255u) / 256u), 256, c->stream, d_src, (const uint64_t*)c->xzWork, (uint32_t)nBlocks, c->xzWork + nBlocks);
            const hipError_t e1 = hipMemcpyAsync(stored.data(), c->xzWork + nBlocks, nBlocks * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream), e2 = hipStreamSynchronize(c->stream);      // (waited for in any case: `words` is read until then)
            HIPCHK(c, e1); HIPCHK(c, e2);
        }
        // the contents' values: one launch per kind of check (a file has one kind unless streams of different kinds were concatenated)
        for (int kind = GC_XZ_CHECK_CRC32; kind <= GC_XZ_CHECK_CRC64; kind += GC_XZ_CHECK_CRC64 - GC_XZ_CHECK_CRC32) {
            std::vector<gc_crc_segment> segs; std::vector<size_t> who; std::vector<uint64_t> vals;
            for (size_t i = 0; i < nBlocks; i++) if ((int)blocks[i].check == kind) { const gc_crc_segment s = { blocks[i].dst_off, blocks[i].dst_size }; segs.push_back(s); who.push_back(i); }
            if ((rc = xz_checks_run(c, kind, d_dst, segs, vals)) != GC_OK) return rc;
            for (size_t k = 0; k < who.size(); k++)
                if (vals[k] != stored[who[k]]) {
                    snprintf(c->err, sizeof(c->err), "xz block %zu: the content's CRC-%d is %0*llx, the file states %0*llx", who[k], kind == GC_XZ_CHECK_CRC32 ? 32 : 64, kind == GC_XZ_CHECK_CRC32 ? 8 : 16,
                             (unsigned long long)vals[k], kind == GC_XZ_CHECK_CRC32 ? 8 : 16, (unsigned long long)stored[who[k]]);
                    return GC_ERR_CORRUPT;
                }
        }
    }
    *outSize = (size_t)total;
    return GC_OK;
}

extern "C" int gc_xz_decompress_device(gc_ctx* c, const void* d_src, size_t n, void* d_dst, size_t dstCap, const gc_xz_block* blocks, size_t nBlocks,
                                       const gc_lzma2_unit* units, size_t nUnits, size_t* outSize)
{
    if (!c || (!d_src && n) || (!blocks && nBlocks) || (!units && nUnits) || !outSize) return GC_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    return xz_decode(c, (const uint8_t*)d_src, nullptr, n, (uint8_t*)d_dst, dstCap, blocks, nBlocks, units, nUnits, outSize);
}

extern "C" int gc_xz_decompress_host(gc_ctx* c, const void* src, size_t n, void* dst, size_t dstCap, size_t* outSize)
{
    if (!c || (!src && n) || (!dst && dstCap)) return GC_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    if (outSize) *outSize = 0;
    if (!n) { snprintf(c->err, sizeof(c->err), "not an xz file: no bytes"); return GC_ERR_CORRUPT; }
    std::vector<gc_xz_block> bl; std::vector<gc_lzma2_unit> un; uint64_t total = 0;
    int rc = xz_scan((const uint8_t*)src, n, bl, un, &total);
    if (rc != GC_OK) { snprintf(c->err, sizeof(c->err), rc == GC_ERR_UNSUPPORTED ? "an xz file with a filter chain or a check this decoder does not handle" : "not a whole xz file (container scan failed)"); return rc; }
    if (total > dstCap) { snprintf(c->err, sizeof(c->err), "destination too small: need %llu bytes", (unsigned long long)total); return GC_ERR_DST_SMALL; }
    return decode_staged(c, rc, src, n, dst, (size_t)total, outSize, [&](size_t* produced) {
        return xz_decode(c, c->dIn, (const uint8_t*)src, n, c->dOut, (size_t)total, bl.data(), bl.size(), un.data(), un.size(), produced); });
}

extern "C" int gc_xz_timing(gc_ctx* c, float ms[2]) { if (!c || !ms) return GC_ERR_PARAM; ms[0] = c->xzMs[0]; ms[1] = c->xzMs[1]; return GC_OK; }
extern "C" int gc_xz_launch_counts(gc_ctx* c, unsigned n[3]) { if (!c || !n) return GC_ERR_PARAM; for (int i = 0; i < 3; i++) n[i] = c->xzCounts[i]; return GC_OK; }

// ------------------------------------------------------------------------------------------------ encoder
static size_t xz_block_bytes(size_t blockBytes, int level) { return blockBytes ? blockBytes : gc_multi_piece_bytes(GC_CODEC_FLZMA2, level); }
// the Block Header's size for a Block of `len` input bytes: fixed BEFORE the Block is coded (its payload is written straight behind it), so the packed size's field is given
// the room of the largest value it can take and Header Padding takes up what the real one leaves
static size_t xz_header_size(size_t len) { return ((2u + xz_vli_len(gc_flzma2_compress_bound(len)) + xz_vli_len(len) + 3u + 3u) & ~(size_t)3u) + 4u; }

extern "C" size_t gc_xz_compress_bound(size_t n, size_t blockBytes)
{
    size_t B = blockBytes;
    if (!B) { B = gc_multi_piece_bytes(GC_CODEC_FLZMA2, 1); for (int lv = 2; lv <= 9; lv++) { const size_t b = gc_multi_piece_bytes(GC_CODEC_FLZMA2, lv); if (b < B) B = b; } }
    const size_t whole = n / B, rest = n - whole * B, nb = whole + (rest ? 1u : 0u);
    // per Block: header, payload, padding, check, Index record; per stream: header, footer, Index indicator + count + padding + CRC
    return whole * gc_flzma2_compress_bound(B) + (rest ? gc_flzma2_compress_bound(rest) : 0u) + nb * (XZ_HEADER_MAX + 3u + 8u + 18u) + 12u + 12u + 20u;
}

extern "C" int gc_xz_compress_device(gc_ctx* c, const void* d_src, size_t n, void* d_dst, size_t dstCap, int level, size_t blockBytes, int check, size_t* outSize)
{
    if (!c || (!d_src && n) || !d_dst || !outSize) return GC_ERR_PARAM;
    if (check != GC_XZ_CHECK_NONE && check != GC_XZ_CHECK_CRC32 && check != GC_XZ_CHECK_CRC64) { snprintf(c->err, sizeof(c->err), "xz check id %d: this encoder writes none (0), CRC-32 (1) or CRC-64 (4)", check); return GC_ERR_PARAM; }
    if (blockBytes && blockBytes < 4096u) { snprintf(c->err, sizeof(c->err), "xz blocks of %zu bytes: at least 4096", blockBytes); return GC_ERR_PARAM; }
    HIPCHK(c, hipSetDevice(c->device));
    *outSize = 0;
    c->xzMs[0] = c->xzMs[1] = 0.f; c->xzCounts[0] = c->xzCounts[1] = c->xzCounts[2] = 0u;
    const size_t B = xz_block_bytes(blockBytes, level), nb = n ? (n + B - 1u) / B : 0u, checkSize = xz_check_size((uint32_t)check);
    const uint8_t* const src = (const uint8_t*)d_src; uint8_t* const dst = (uint8_t*)d_dst;
    const uint8_t prop = gc_flzma2_dict_prop(level);
    int rc = xz_events(c);
    if (rc != GC_OK) return rc;
    // the Checks of all Blocks: one launch over the input where it lies
    std::vector<uint64_t> checks;
    if (check != GC_XZ_CHECK_NONE) {
        std::vector<gc_crc_segment> segs(nb);
        for (size_t i = 0; i < nb; i++) { segs[i].offset = i * B; segs[i].length = (i + 1u) * B <= n ? B : n - i * B; }
        if ((rc = xz_checks_run(c, check, src, segs, checks)) != GC_OK) return rc;
    }
    // what the host writes -- headers, padding + Check, Index, footer -- is put together in ONE array that lives until the stream has been waited for: the copies read it
    std::vector<uint8_t> meta(12u + nb * (XZ_HEADER_MAX + 3u + 8u + 18u) + 12u + 20u, 0u);
    std::vector<uint64_t> recs; recs.reserve(nb * 2u);
    size_t at = 0, pos = 0;
    const auto put = [&](size_t bytes) -> int {        // meta[at, at + bytes) -> dst[pos ...]
        if (bytes > dstCap - pos) { snprintf(c->err, sizeof(c->err), "destination too small: the xz stream needs more than %zu bytes", dstCap); return GC_ERR_DST_SMALL; }
        if (bytes) HIPCHK(c, hipMemcpyAsync(dst + pos, meta.data() + at, bytes, hipMemcpyHostToDevice, c->stream));
        at += bytes; pos += bytes;
        return GC_OK;
    };
    const auto run = [&]() -> int {
        int r;
        uint8_t* m = meta.data();
        memcpy(m, kXzMagic, 6); m[6] = 0u; m[7] = (uint8_t)check; xz_put32(m + 8, xz_crc32(m + 6, 2));
        if ((r = put(12u)) != GC_OK) return r;
        for (size_t i = 0; i < nb; i++) {
            const size_t off = i * B, len = (i + 1u) * B <= n ? B : n - off, H = xz_header_size(len);
            if (H >= dstCap - pos) { snprintf(c->err, sizeof(c->err), "destination too small: the xz stream needs more than %zu bytes", dstCap); return GC_ERR_DST_SMALL; }
            // the Block's LZMA2 stream, straight to its place behind the header: a stream of its own (dictionary reset at its start, end marker at its end)
            size_t packed = 0; float ms[7];
            if ((r = gc_flzma2_compress_device(c, src + off, len, dst + pos + H, dstCap - pos - H, level, 0u)) != GC_OK) return r;
            if ((r = gc_flzma2_finish(c, &packed)) != GC_OK) return r;
            if (gc_flzma2_last_timing(c, ms) == GC_OK) c->xzMs[0] += ms[6];
            m = meta.data() + at;
            size_t k = 0;
            m[k++] = (uint8_t)(H / 4u - 1u); m[k++] = 0xC0u;                   // one filter, both sizes present
            k += xz_put_vli(m + k, packed); k += xz_put_vli(m + k, len);
            m[k++] = 0x21u; m[k++] = 1u; m[k++] = prop;
            xz_put32(m + H - 4u, xz_crc32(m, H - 4u));                         // (Header Padding: the array starts as zeros)
            if ((r = put(H)) != GC_OK) return r;
            pos += packed;                                                     // (inside the capacity: the encoder was given what is left of it)
            m = meta.data() + at;
            const size_t pad = (4u - (packed & 3u)) & 3u;
            for (size_t b = 0; b < checkSize; b++) m[pad + b] = (uint8_t)(checks[i] >> (8u * b));
            if ((r = put(pad + checkSize)) != GC_OK) return r;
            recs.push_back(H + packed + checkSize); recs.push_back(len);
        }
        m = meta.data() + at;
        size_t k = 0;
        m[k++] = 0u; k += xz_put_vli(m + k, nb);
        for (size_t i = 0; i < recs.size(); i++) k += xz_put_vli(m + k, recs[i]);
        k = (k + 3u) & ~(size_t)3u;
        xz_put32(m + k, xz_crc32(m, k)); k += 4u;
        uint8_t* f = m + k;
        xz_put32(f + 4, (uint32_t)(k / 4u - 1u)); f[8] = 0u; f[9] = (uint8_t)check; f[10] = 0x59u; f[11] = 0x5Au; xz_put32(f, xz_crc32(f + 4, 6));
        return put(k + 12u);
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(c->stream);                     // (whatever happened: the copies read `meta`)
    if (rc == GC_OK) HIPCHK(c, e);
    if (rc != GC_OK) return rc;
    *outSize = pos;
    return GC_OK;
}

extern "C" int gc_xz_compress_host(gc_ctx* c, const void* src, size_t n, void* dst, size_t dstCap, int level, size_t blockBytes, int check, size_t* outSize)
{
    if (!c || (!src && n) || !dst || !outSize) return GC_ERR_PARAM;
    if (blockBytes && blockBytes < 4096u) { snprintf(c->err, sizeof(c->err), "xz blocks of %zu bytes: at least 4096", blockBytes); return GC_ERR_PARAM; }
    HIPCHK(c, hipSetDevice(c->device));
    *outSize = 0;
    if (stage_reserve(c, n, gc_xz_compress_bound(n, xz_block_bytes(blockBytes, level)), 0u) != GC_OK) return GC_ERR_NOMEM;
    if (n) HIPCHK(c, hipMemcpyAsync(c->dIn, src, n, hipMemcpyHostToDevice, c->stream));      // the input crosses the link once: checks and blocks read it from there
    size_t sz = 0;
    const int rc = gc_xz_compress_device(c, c->dIn, n, c->dOut, c->dOut.cap, level, blockBytes, check, &sz);
    if (rc != GC_OK) return rc;
    if (sz > dstCap) { snprintf(c->err, sizeof(c->err), "destination too small: need %zu bytes", sz); return GC_ERR_DST_SMALL; }
    HIPCHK(c, hipMemcpyAsync(dst, c->dOut, sz, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *outSize = sz;
    return GC_OK;
}
