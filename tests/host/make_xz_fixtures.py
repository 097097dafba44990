"""tests/host/make_xz_fixtures.py DIR -- TEST INFRASTRUCTURE ONLY: writes the .xz files that tests/test_xz.py feeds the decoder (foreign single-block streams, multi-block files
assembled from raw LZMA2 streams, concatenated streams, padding, refusals) into DIR for tests/host/xz_container.cpp: NAME.xz with NAME.bin (the content a decoder must give)
or NAME.rc (the error code it must return)."""
import lzma
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import xz_cases as X


def main(out):
    os.makedirs(out, exist_ok=True)
    rng = np.random.default_rng(3)
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(200)]
    text = b" ".join(words[int(i)] for i in rng.integers(0, 200, size=6000))
    x = text[:20_000] + bytes(rng.integers(0, 256, size=3000, dtype=np.uint8)) + bytes(4000) + text[:9000]

    def good(name, stream, content):
        open(os.path.join(out, name + ".xz"), "wb").write(stream); open(os.path.join(out, name + ".bin"), "wb").write(content)

    def bad(name, stream, rc):
        open(os.path.join(out, name + ".xz"), "wb").write(stream); open(os.path.join(out, name + ".rc"), "w").write(str(rc))
    for check in X.ENC_CHECKS:
        for preset in (0, 6, 9):
            good("lzma_%s_p%d" % (check, preset), lzma.compress(x, check=X.LZMA_CHECKS[check], preset=preset), x)
        for lc, lp, pb in ((4, 0, 0), (0, 2, 2)):
            good("lzma_%s_%d%d%d" % (check, lc, lp, pb), lzma.compress(x, check=X.LZMA_CHECKS[check], filters=[{"id": lzma.FILTER_LZMA2, "preset": 6, "lc": lc, "lp": lp, "pb": pb}]), x)
    for nb in (1, 2, 37):
        s, _ = X.build_stream(X.split_parts(x, nb), "crc64")
        assert lzma.decompress(s) == x
        good("blocks_%d" % nb, s, x)
    a, _ = X.build_stream(X.split_parts(x, 3), "crc64"); b, lay = X.build_stream(X.split_parts(x[:7000], 2), "crc32")
    good("two_streams", a + b, x + x[:7000])
    good("padding_4_8", a + bytes(4) + b + bytes(8), x + x[:7000])
    good("zero_blocks", X.build_stream([], "crc64")[0], b"")
    flip = lambda s, at, bit: s[:at] + bytes([s[at] ^ (1 << bit)]) + s[at + 1:]
    bad("flip_check", flip(b, lay[0]["check_off"], 2), -6)
    bad("flip_block_header", flip(b, 14, 0), -6)
    bad("flip_index_crc", flip(b, len(b) - 14, 1), -6)
    bad("flip_footer", flip(b, len(b) - 6, 0), -6)
    bad("truncated", a[:len(a) - 7], -6)
    bad("padding_3", a + bytes(3) + b, -6)
    bad("sha256", lzma.compress(x, check=lzma.CHECK_SHA256), -7)
    bad("delta", lzma.compress(x, filters=[{"id": lzma.FILTER_DELTA, "dist": 4}, {"id": lzma.FILTER_LZMA2, "preset": 6}]), -7)


if __name__ == "__main__":
    main(sys.argv[1])
