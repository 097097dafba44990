"""The cases of tests/test_scatter_stable.py, shared with tools/gen_scatter_golden.py (which records their hashes at another commit).

zstd levels 3 (fast geometry: 256 partitions, 8 KiB tiles) and 19, Fast-LZMA2 level 5 and brotli quality 6 (wide geometry: 1024 partitions,
16 KiB tiles; far, far2 and short instantiations of the shared body)
  * on text at the edge sizes 1 B, one tile +- 1, one block +- 1 -- ONE block, which the block-local finder takes: these check that the
    short path is untouched, the scatter pass does not run for them;
  * on text at two blocks and a tile-edge tail (8 KiB +- 1, 16 KiB +- 1): the windowed finder with a partial, a whole and a just-started
    last tile in either geometry;
  * on text at one finder frame +- 1 and at two frames and a part;
  * on each generator corpus at two blocks and a part."""
import hashlib

import numpy as np

BLK = 128 * 1024
FRAME = 64 * BLK

CODECS = (("zstd", 3), ("zstd", 19), ("flzma2", 5), ("brotli", 6))
KINDS = ("text-zipf", "web-text", "lz-7zip", "silesia-like", "random", "zeros")
ONE_BLOCK_SIZES = (1, 8191, 8192, 8193, 16383, 16384, 16385, BLK - 1, BLK, BLK + 1)
TILE_TAIL_SIZES = tuple(2 * BLK + t for t in (8191, 8192, 8193, 16383, 16384, 16385))
FRAME_SIZES = (FRAME - 1, FRAME, FRAME + 1, 2 * FRAME + 12345)
CORPUS_SIZE = 2 * BLK + 1234


def cases():
    """(codec, level, corpus kind, bytes) of every case; the emulator and the device run the same ones."""
    out = []
    for codec, level in CODECS:
        out += [(codec, level, "text-zipf", n) for n in ONE_BLOCK_SIZES + TILE_TAIL_SIZES + FRAME_SIZES]
        out += [(codec, level, kind, CORPUS_SIZE) for kind in KINDS]
    return out


def case_id(case):
    return "%s-%d/%s/%d" % case


def stream_sha256(pkg, corpus, case, **enc_kw):
    """Compress the case's input with a fresh encoder (lib_path=<emulator library> or device=<n>) and hash the stream."""
    codec, level, kind, n = case
    cls = {"zstd": pkg.ZstdEncoder, "flzma2": pkg.Flzma2Encoder, "brotli": pkg.BrotliEncoder}[codec]
    enc = cls(level=level, **enc_kw)
    try:
        c = enc.code(corpus(kind, n))
    finally:
        enc.close()
    return hashlib.sha256(np.ascontiguousarray(c, dtype=np.uint8).tobytes()).hexdigest()
