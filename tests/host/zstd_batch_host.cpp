// tests/host/zstd_batch_host.cpp -- TEST INFRASTRUCTURE ONLY: the batched zstd encoder through the C ABI -- sizes at every boundary, placement, rounds, refusals and
// edges (cases 1, 2, 7 and 8 of tests/test_zstd_batch.py) -- then gc_ctx_destroy.  Linked against the AddressSanitizer build of the emulator library (`make -C
// tests/host -f zstd_batch_host.mk`) and run with leak detection on: exit status 0 = every frame equal to the stream call's, every refusal as documented, no read or write
// outside a buffer (the inputs are exact-size heap blocks, so a read past an item's buffer is a report) and nothing left allocated.
#include "gpucodec.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>

typedef std::vector<uint8_t> Bytes;
typedef std::vector<gc_batch_item> Items;
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static Bytes make_input(size_t n, uint32_t seed)
{
    static const char* words[] = { "the", "block", "parallel", "match", "finder", "window", "of", "frame", "and", "literal", "sequence", "stream", "device", "buffer", "range", "coder" };
    Bytes b; b.reserve(n + 16);
    uint32_t s = seed;
    while (b.size() < n) {
        s = s * 1664525u + 1013904223u;
        const char* w = words[(s >> 24) & 15u];
        b.insert(b.end(), w, w + strlen(w));
        b.push_back((s >> 20) & 15u ? ' ' : '\n');
        if (((s >> 8) & 63u) == 0u) for (int i = 0; i < 6; i++) { s = s * 1664525u + 1013904223u; b.push_back((uint8_t)(s >> 24)); }
    }
    b.resize(n);
    return b;
}

static Bytes stream_call(gc_ctx* one, const uint8_t* p, size_t n)
{
    Bytes out(gc_zstd_compress_bound(n));
    size_t sz = 0;
    const int rc = gc_zstd_compress_host(one, p, n, out.data(), out.size(), 3, &sz);
    CHECK(rc == GC_OK, "stream call on %zu bytes: %d (%s)", n, rc, gc_last_error_message(one));
    out.resize(rc == GC_OK ? sz : 0);
    return out;
}

// one batch over `src` (the emulator's device memory is host memory: an exact-size copy, so the sanitizer sees every read outside it): -> packed output and results
static bool batch_call(gc_ctx* c, const Bytes& src, const Items& items, Bytes& out, std::vector<gc_batch_result>& res, const char* what)
{
    Bytes dst(gc_zstd_batch_compress_bound(items.data(), items.size()) + 1u);
    res.assign(items.size() + 1u, gc_batch_result());
    size_t total = 0;
    int rc = gc_zstd_batch_compress_device(c, src.data(), src.size(), items.data(), items.size(), dst.data(), dst.size() - 1u, 3);
    CHECK(rc == GC_OK, "%s: batch call: %d (%s)", what, rc, gc_last_error_message(c));
    if (rc != GC_OK) return false;
    rc = gc_zstd_batch_finish(c, res.data(), &total);
    CHECK(rc == GC_OK, "%s: finish: %d (%s)", what, rc, gc_last_error_message(c));
    if (rc != GC_OK) return false;
    out.assign(dst.begin(), dst.begin() + total);
    return true;
}

// the contract: results[i] cuts out the stream call's bytes for item i, frames packed in order; the whole output decodes to the items concatenated
static void check_batch(gc_ctx* c, gc_ctx* one, const Bytes& src, const Items& items, const char* what)
{
    Bytes out; std::vector<gc_batch_result> res;
    if (!batch_call(c, src, items, out, res, what)) return;
    size_t pos = 0; Bytes content;
    for (size_t i = 0; i < items.size(); i++) {
        const uint8_t* p = src.data() + items[i].src_off;
        const Bytes want = stream_call(one, p, items[i].src_size);
        CHECK(res[i].dst_off == pos && res[i].dst_size == want.size() && pos + want.size() <= out.size() && !memcmp(out.data() + pos, want.data(), want.size()),
              "%s: item %zu (%u bytes at %llu): frame of %u bytes at %llu, the stream call gives %zu at %zu", what, i, items[i].src_size, (unsigned long long)items[i].src_off,
              res[i].dst_size, (unsigned long long)res[i].dst_off, want.size(), pos);
        pos += want.size();
        content.insert(content.end(), p, p + items[i].src_size);
    }
    CHECK(pos == out.size(), "%s: %zu bytes of frames, total %zu", what, pos, out.size());
    Bytes got(content.size() + 1u);
    size_t sz = 0;
    const int rc = gc_zstd_decompress_host(one, out.data(), out.size(), got.data(), content.size(), &sz);
    CHECK(rc == GC_OK && sz == content.size() && !memcmp(got.data(), content.data(), content.size()), "%s: decoding the packed output: %d, %zu of %zu bytes", what, rc, sz, content.size());
}

static Items packed_items(const std::vector<uint32_t>& sizes)
{
    Items it; uint64_t off = 0;
    for (uint32_t n : sizes) { gc_batch_item x; x.src_off = off; x.src_size = n; x.reserved = 0; it.push_back(x); off += n; }
    return it;
}
static gc_batch_item item(uint64_t off, uint32_t n) { gc_batch_item x; x.src_off = off; x.src_size = n; x.reserved = 0; return x; }

int main()
{
    gc_ctx *c = nullptr, *one = nullptr;
    if (gc_ctx_create(&c, 0) != GC_OK || gc_ctx_create(&one, 0) != GC_OK) { fprintf(stderr, "gc_ctx_create failed\n"); return 2; }
    const uint32_t BLK = GC_ZSTD_BATCH_ITEM_MAX;

    {   // case 1: sizes at every boundary the kernels have (64 = the finder's match cap: a position hashes once cap + 16 bytes are readable behind it)
        const std::vector<uint32_t> sizes = { 0, 1, 7, 8, 9, 31, 32, 33, 79, 80, 81, 255, 256, 1023, 1024, 1025, 65791, 65792, BLK - 1u, BLK };
        const Items items = packed_items(sizes);
        const Bytes src = make_input((size_t)(items.back().src_off + items.back().src_size), 1u);
        check_batch(c, one, src, items, "boundaries");
        gc_ctx_set_option(c, GC_OPT_ZSTD_CHECKSUM, 1); gc_ctx_set_option(one, GC_OPT_ZSTD_CHECKSUM, 1);
        check_batch(c, one, src, Items(items.begin(), items.begin() + 17), "boundaries with checksums");
        gc_ctx_set_option(c, GC_OPT_ZSTD_CHECKSUM, 0); gc_ctx_set_option(one, GC_OPT_ZSTD_CHECKSUM, 0);
    }
    const Bytes src = make_input(40000, 2u);
    const Items placed = { item(1, 3001), item(3003, 2000), item(9100, 5000), item(20001, 6000), item(23000, 6000), item(30001, 4000), item(30001, 4000),
                           item(34000, 6000) /* ends with the buffer */, item(23000, 6000), item(20001, 6000), item(9100, 5000), item(3003, 2000), item(1, 3001) };
    check_batch(c, one, src, placed, "placement");      // case 2: odd offsets, gaps of 1 and 4097, overlap, a repeat, descending order

    {   // case 7: rounds of 3 + 3 + 2 and of one item give the bytes and the table of one round
        const Items items = packed_items({ 1500, 0, 2500, 700, 9000, 33, 4000, 1200 });
        Bytes ref, got; std::vector<gc_batch_result> rref, rgot;
        if (batch_call(c, src, items, ref, rref, "one round")) {
            for (const char* r : { "3", "1" }) {
                setenv("GC_BATCH_ROUND_ITEMS", r, 1);
                if (batch_call(c, src, items, got, rgot, "small rounds"))
                    CHECK(got == ref && !memcmp(rgot.data(), rref.data(), items.size() * sizeof(gc_batch_result)), "rounds of %s items: other bytes or another table", r);
                check_batch(c, one, src, items, "small rounds");
                unsetenv("GC_BATCH_ROUND_ITEMS");
            }
        }

        // case 8: refusals and edges
        Bytes dst(gc_zstd_batch_compress_bound(items.data(), items.size()), 0xA5);
        const Bytes big = make_input(BLK + 1000u, 3u);
        const Items tooBig = { item(0, 100), item(7, BLK + 1u) };
        CHECK(gc_zstd_batch_compress_device(c, big.data(), big.size(), tooBig.data(), 2, dst.data(), dst.size(), 3) == GC_ERR_PARAM
              && strstr(gc_last_error_message(c), "item 1") && strstr(gc_last_error_message(c), "131073"), "an item above one block: %s", gc_last_error_message(c));
        const Items outside = { item(0, 100), item(src.size() - 99u, 100) };
        CHECK(gc_zstd_batch_compress_device(c, src.data(), src.size(), outside.data(), 2, dst.data(), dst.size(), 3) == GC_ERR_PARAM
              && strstr(gc_last_error_message(c), "item 1"), "an item behind the input: %s", gc_last_error_message(c));
        size_t total = 1;
        CHECK(gc_zstd_batch_finish(c, nullptr, &total) == GC_ERR_PARAM, "finish without a pending batch");
        CHECK(gc_zstd_batch_compress_device(c, nullptr, 0, nullptr, 0, nullptr, 0, 3) == GC_OK && gc_zstd_batch_finish(c, nullptr, &total) == GC_OK && total == 0, "an empty batch");
        CHECK(gc_zstd_batch_compress_device(c, src.data(), src.size(), items.data(), items.size(), dst.data(), ref.size() - 1u, 3) == GC_OK, "batch into a short destination");
        CHECK(gc_zstd_batch_finish(c, rgot.data(), &total) == GC_ERR_DST_SMALL, "a destination one byte short");
        bool untouched = true; for (uint8_t b : dst) untouched &= b == 0xA5;
        CHECK(untouched, "a short destination was written to");
        check_batch(c, one, src, items, "after the refusals");
        // the host entry: gathered inputs, exact-size heap blocks
        std::vector<Bytes> parts; std::vector<const void*> ptrs; std::vector<size_t> sizes;
        for (const gc_batch_item& it : items) parts.push_back(Bytes(src.begin() + it.src_off, src.begin() + it.src_off + it.src_size));
        for (const Bytes& p : parts) { ptrs.push_back(p.data()); sizes.push_back(p.size()); }
        Bytes hostOut(ref.size());
        CHECK(gc_zstd_batch_compress_host(c, ptrs.data(), sizes.data(), parts.size(), hostOut.data(), hostOut.size(), 3, rgot.data(), &total) == GC_OK && total == ref.size() && hostOut == ref,
              "host entry: %s", gc_last_error_message(c));
        // a stream call after a batch call, and a batch call after a stream call
        CHECK(stream_call(c, src.data(), src.size()) == stream_call(one, src.data(), src.size()), "stream call after a batch call");
        check_batch(c, one, src, items, "batch call after a stream call");
        float ms[4] = { -1.f, -1.f, -1.f, -1.f };
        CHECK(gc_zstd_batch_timing(c, ms) == GC_OK && ms[0] >= 0.f && ms[3] >= 0.f, "batch timing");
        // ... and a batch left pending when its context goes
        CHECK(gc_zstd_batch_compress_device(c, src.data(), src.size(), items.data(), items.size(), dst.data(), dst.size(), 3) == GC_OK, "last batch call");
    }
    gc_ctx_destroy(c);
    gc_ctx_destroy(one);
    printf("zstd_batch_host: %d failed checks\n", failures);
    return failures ? 1 : 0;
}
