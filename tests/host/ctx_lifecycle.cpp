// tests/host/ctx_lifecycle.cpp -- TEST INFRASTRUCTURE ONLY: one gc_ctx through every path that grows a device buffer, then gc_ctx_destroy.
// Linked against the AddressSanitizer build of the emulator library (tests/emu: `make lifecycle`) and run with leak detection on, it is the check that
// whatever a context allocates is released with it: exit status 0 = every round trip equal and no report of the sanitizer.
#include "gpucodec.h"
#include <chrono>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>

typedef std::vector<uint8_t> Bytes;
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// text-like bytes: words drawn from a small vocabulary, so that the finder has matches at every distance
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

static const int kCodecs[3] = { GC_CODEC_ZSTD, GC_CODEC_FLZMA2, GC_CODEC_BROTLI };
static const int kLevels[3] = { 5, 5, 6 };                       // the levels whose parse is the priced one: every finder array is in play
static const char* const kNames[3] = { "zstd", "flzma2", "brotli" };

static Bytes compress(gc_ctx* c, int k, const Bytes& in, unsigned flags = 0)
{
    Bytes out(gc_codec_compress_bound(kCodecs[k], in.size()));
    size_t sz = 0;
    const int rc = gc_codec_compress_host(c, kCodecs[k], in.data(), in.size(), out.data(), out.size(), kLevels[k], flags, &sz);
    CHECK(rc == GC_OK, "%s: compressing %zu bytes: %d (%s)", kNames[k], in.size(), rc, gc_last_error_message(c));
    out.resize(rc == GC_OK ? sz : 0);
    return out;
}

static void round_trip(gc_ctx* c, int k, const Bytes& comp, const Bytes& want, const char* what)
{
    Bytes got(want.size());
    size_t sz = 0;
    const int rc = kCodecs[k] == GC_CODEC_ZSTD ? gc_zstd_decompress_host(c, comp.data(), comp.size(), got.data(), got.size(), &sz)
                 : kCodecs[k] == GC_CODEC_BROTLI ? gc_brotli_decompress_host(c, comp.data(), comp.size(), got.data(), got.size(), &sz)
                 : gc_lzma2_decompress_host(c, comp.data(), comp.size(), got.data(), got.size(), gc_flzma2_dict_prop(kLevels[k]), &sz);
    CHECK(rc == GC_OK, "%s (%s): decoding: %d (%s)", kNames[k], what, rc, gc_last_error_message(c));
    CHECK(sz == want.size() && got == want, "%s (%s): %zu bytes came back, %zu went in, content %s", kNames[k], what, sz, want.size(), got == want ? "equal" : "DIFFERENT");
}

static void filter_round_trip(gc_ctx* c, int kind, unsigned delta, const Bytes& in)
{
    Bytes data = in;
    unsigned char state[256];
    size_t done = 0, undone = 0;
    memset(state, 0, sizeof(state));
    int rc = gc_filter_host(c, kind, data.data(), data.size(), 0u, 1, delta, state, &done);
    CHECK(rc == GC_OK, "filter %d encoding: %d (%s)", kind, rc, gc_last_error_message(c));
    memset(state, 0, sizeof(state));
    rc = gc_filter_host(c, kind, data.data(), data.size(), 0u, 0, delta, state, &undone);
    CHECK(rc == GC_OK, "filter %d decoding: %d (%s)", kind, rc, gc_last_error_message(c));
    CHECK(done == undone && data == in, "filter %d: %zu bytes converted, %zu converted back, content %s", kind, done, undone, data == in ? "equal" : "DIFFERENT");
}

int main(int argc, char** argv)
{
    const auto t0 = std::chrono::steady_clock::now();
    // (`ctx_lifecycle small`: 2 blocks + 1 byte as the large input, where the emulator is too slow for more -- still three blocks, and two frames under GC_FRAME_BLOCKS=2)
    const bool less = argc > 1 && !strcmp(argv[1], "small");
    const Bytes small = make_input(1000, 1u), large = make_input(less ? 2u * 128u * 1024u + 1u : 3u * 128u * 1024u + 12345u, 2u);
    gc_ctx* c = nullptr;
    int rc = gc_ctx_create(&c, 0);
    if (rc != GC_OK || !c) { fprintf(stderr, "gc_ctx_create: %d\n", rc); return 2; }

    // small (one block: the block-local finder), large (the per-block workspace and every finder array grow), small again (nothing shrinks)
    std::vector<std::pair<Bytes, const Bytes*>> streams[3];
    const Bytes* const order[3] = { &small, &large, &small };
    for (int step = 0; step < 3; step++)
        for (int k = 0; k < 3; k++) streams[k].push_back({ compress(c, k, *order[step]), order[step] });
    for (int k = 0; k < 3; k++) CHECK(streams[k][0].first == streams[k][2].first, "%s: the small input compresses differently after the large one", kNames[k]);

    // the multi-part path (arrays sized for the largest part): the hooks are read by gc_ctx_create, so this leg has a context of its own beside the first
    {
        setenv("GC_FRAME_BLOCKS", "2", 1); setenv("GC_PART_FRAMES", "1", 1);
        gc_ctx* p = nullptr;
        rc = gc_ctx_create(&p, 0);
        unsetenv("GC_FRAME_BLOCKS"); unsetenv("GC_PART_FRAMES");
        CHECK(rc == GC_OK && p, "gc_ctx_create under GC_FRAME_BLOCKS / GC_PART_FRAMES: %d", rc);
        if (p) {
            for (int k = 0; k < 3; k++) { const Bytes comp = compress(p, k, large); round_trip(c, k, comp, large, "parts"); }
            gc_ctx_destroy(p);
        }
    }

    // content checksums: the per-frame hash array
    {
        CHECK(gc_ctx_set_option(c, GC_OPT_ZSTD_CHECKSUM, 1) == GC_OK, "GC_OPT_ZSTD_CHECKSUM");
        const Bytes comp = compress(c, 0, large);
        CHECK(gc_ctx_set_option(c, GC_OPT_ZSTD_CHECKSUM, 0) == GC_OK, "GC_OPT_ZSTD_CHECKSUM off");
        round_trip(c, 0, comp, large, "checksums");
    }

    // every stream back through the host-buffer decoders of the same context
    for (int k = 0; k < 3; k++)
        for (size_t i = 0; i < streams[k].size(); i++) round_trip(c, k, streams[k][i].first, *streams[k][i].second, i == 1 ? "large" : "small");

    // the filters' staging
    const Bytes code = make_input(70000, 3u);
    filter_round_trip(c, GC_FILTER_X86, 0u, code);
    filter_round_trip(c, GC_FILTER_DELTA, 4u, code);

    gc_ctx_destroy(c);
    // ... and a context that was never used
    c = nullptr;
    rc = gc_ctx_create(&c, 0);
    CHECK(rc == GC_OK && c, "second gc_ctx_create: %d", rc);
    gc_ctx_destroy(c);

    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("ctx_lifecycle: %s, %d failed checks, %.1f s\n", less ? "2 blocks + 1" : "3 blocks + 12345", failures, s);
    return failures ? 1 : 0;
}
