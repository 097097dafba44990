// tests/host/xz_container.cpp -- TEST INFRASTRUCTURE ONLY: the .xz reader (csrc/gc_xz.h: container scan, LZMA2 chunk scan, decode, checks) as a plain program for the
// sanitizers.  Compiled together with the emulator build of the library's sources, all of it with -fsanitize=address,undefined, and run as an ordinary executable:
//     xz_container DIR      DIR: the files of tests/host/make_xz_fixtures.py (NAME.xz with NAME.bin = the content, or NAME.rc = the error code)
// Every fixture must decode to its content or give its error code; then 2 000 randomly damaged variants of one small file of this engine's own encoder must each give
// an error or the right bytes.  Exit status 0 = all of that and no report of a sanitizer.
#include "gpucodec.h"
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static bool read_file(const std::string& path, Bytes& out)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

// scan (count, then fill) + decode; the scan's total is the capacity.  -> the error code; `got` = the content
static int decode(gc_ctx* c, const Bytes& s, Bytes& got)
{
    got.clear();
    size_t nb = 0, nu = 0; uint64_t total = 0;
    int rc = gc_xz_scan(s.data(), s.size(), nullptr, 0, &nb, nullptr, 0, &nu, &total);
    if (rc != GC_OK) return rc;
    std::vector<gc_xz_block> blocks(nb + 1); std::vector<gc_lzma2_unit> units(nu + 1);
    size_t nb2 = 0, nu2 = 0; uint64_t total2 = 0;
    rc = gc_xz_scan(s.data(), s.size(), blocks.data(), nb, &nb2, units.data(), nu, &nu2, &total2);
    CHECK(rc == GC_OK && nb2 == nb && nu2 == nu && total2 == total, "the second scan differs from the first: %d", rc);
    if (rc != GC_OK) return rc;
    for (size_t i = 0; i < nb; i++)
        CHECK(blocks[i].src_off + blocks[i].src_size <= s.size() && blocks[i].check_off + 8u <= s.size() + 8u && blocks[i].dst_off + blocks[i].dst_size <= total, "block %zu lies outside the file", i);
    for (size_t i = 0; i < nu; i++) CHECK(units[i].src_off + units[i].src_size <= s.size() && units[i].dst_off + units[i].dst_size <= total, "unit %zu lies outside the file", i);
    if (total > (64u << 20)) return GC_ERR_DST_SMALL;                 // (a damaged size field: the decoder is not asked for that much)
    got.assign((size_t)total + 1u, 0xA5);
    size_t sz = 0;
    rc = gc_xz_decompress_host(c, s.data(), s.size(), got.data(), (size_t)total, &sz);
    CHECK(got[(size_t)total] == 0xA5, "a byte behind the capacity was written");
    got.resize(rc == GC_OK ? sz : 0);
    return rc;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: xz_container FIXTURE_DIR\n"); return 2; }
    gc_ctx* c = nullptr;
    int rc = gc_ctx_create(&c, 0);
    if (rc != GC_OK || !c) { fprintf(stderr, "gc_ctx_create: %d\n", rc); return 2; }
    // 1. the fixtures
    int nFix = 0;
    if (DIR* d = opendir(argv[1])) {
        while (struct dirent* e = readdir(d)) {
            const std::string name = e->d_name;
            if (name.size() < 4 || name.substr(name.size() - 3) != ".xz") continue;
            const std::string base = std::string(argv[1]) + "/" + name.substr(0, name.size() - 3);
            Bytes s, want, got, code;
            if (!read_file(base + ".xz", s)) continue;
            nFix++;
            rc = decode(c, s, got);
            if (read_file(base + ".bin", want)) CHECK(rc == GC_OK && got == want, "%s: rc %d, %zu bytes, want %zu (%s)", name.c_str(), rc, got.size(), want.size(), gc_last_error_message(c));
            else if (read_file(base + ".rc", code)) { code.push_back(0); CHECK(rc == atoi((const char*)code.data()), "%s: rc %d, want %s", name.c_str(), rc, (const char*)code.data()); }
            else CHECK(false, "%s: neither .bin nor .rc beside it", name.c_str());
        }
        closedir(d);
    }
    CHECK(nFix >= 20, "only %d fixtures in %s", nFix, argv[1]);
    // 2. one small file of the engine's own encoder (three blocks, CRC-64), damaged 2 000 times
    Bytes x(10000);
    uint32_t s32 = 12345u;
    for (size_t i = 0; i < x.size(); i++) { s32 = s32 * 1664525u + 1013904223u; x[i] = (i % 700u) < 500u ? (uint8_t)("the quick brown fox "[i % 20u]) : (uint8_t)(s32 >> 24); }
    Bytes file(gc_xz_compress_bound(x.size(), 4096));
    size_t fsz = 0;
    rc = gc_xz_compress_host(c, x.data(), x.size(), file.data(), file.size(), 5, 4096, GC_XZ_CHECK_CRC64, &fsz);
    CHECK(rc == GC_OK, "gc_xz_compress_host: %d (%s)", rc, gc_last_error_message(c));
    file.resize(fsz);
    Bytes got;
    rc = decode(c, file, got);
    CHECK(rc == GC_OK && got == x, "the undamaged file: rc %d", rc);
    int refused = 0, accepted = 0;
    for (int round = 0; round < 2000; round++) {
        Bytes bad = file;
        const auto rnd = [&]() { s32 = s32 * 1664525u + 1013904223u; return s32 >> 8; };
        switch (round % 5) {
        case 0: bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8u)); break;
        case 1: bad.resize(rnd() % bad.size()); break;
        case 2: { const size_t at = rnd() % (bad.size() - 8u); for (int k = 0; k < 8; k++) bad[at + k] = (uint8_t)rnd(); break; }
        case 3: bad[rnd() % bad.size()] = (uint8_t)rnd(); break;
        default: { const size_t at = rnd() % bad.size(); bad.insert(bad.begin() + at, (size_t)(1u + rnd() % 8u), (uint8_t)0); break; }
        }
        rc = decode(c, bad, got);
        if (rc == GC_OK) { accepted++; CHECK(got == x, "round %d: a damaged file decoded to other bytes", round); }
        else { refused++; CHECK(rc == GC_ERR_CORRUPT || rc == GC_ERR_UNSUPPORTED || rc == GC_ERR_DST_SMALL, "round %d: rc %d", round, rc); }
    }
    CHECK(refused > 1500, "only %d of 2000 damaged files were refused", refused);
    rc = decode(c, file, got);
    CHECK(rc == GC_OK && got == x, "the undamaged file after the damaged ones: rc %d", rc);
    gc_ctx_destroy(c);
    printf("xz_container: %d fixtures, 2000 damaged variants (%d refused, %d harmless), %d failed checks\n", nFix, refused, accepted, failures);
    return failures ? 1 : 0;
}
