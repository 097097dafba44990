"""Regenerates tests/golden/lzma2_xz_vectors.npz: raw LZMA2 streams written by xz's encoder (Python's standard `lzma` module) -- a third, independent encoder
beside the reference's Fast-LZMA2 and this engine's own -- with lc / lp / pb combinations and dictionary sizes the other two never choose, so that the vectors do not
disappear where `lzma` is missing.  Per vector: the stream, its lc / lp / pb, the LZMA2 dictionary property byte, the corpus recipe of the content, the content's size
and SHA-256.

    python tests/golden/make_lzma2_fixture.py
"""
import hashlib
import lzma
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# (lc, lp, pb, dictionary bytes, preset, recipe)
VECTORS = [(3, 0, 2, 4 << 10, 6, "text"), (4, 0, 0, 64 << 10, 9, "text"), (0, 4, 4, 1 << 20, 1, "records"), (2, 2, 1, 16 << 20, 6, "mix"), (3, 0, 2, 1 << 20, 0, "mix")]


def dict_prop(size):
    """the smallest LZMA2 dictionary property byte whose size (LZMA2_DIC_SIZE_FROM_PROP, C/Lzma2Dec.c) holds `size`"""
    for p in range(40):
        if ((2 | (p & 1)) << (p // 2 + 11)) >= size:
            return p
    return 40


def content(O, recipe):
    if recipe == "text":
        return O.corpus("text-zipf", 20_000)
    if recipe == "records":
        return O.corpus("silesia-like", 10_000)
    # text, bytes that do not compress, a long run, text that repeats what lies in front of the run
    t = O.corpus("text-zipf", 12_000)
    return np.concatenate([t, O.corpus("random", 2_000), np.zeros(70_000, dtype=np.uint8), t[:6_000], O.corpus("lz-7zip", 9_000)])


def xz_raw(x, lc, lp, pb, dict_size, preset):
    return lzma.compress(x.tobytes(), format=lzma.FORMAT_RAW,
                         filters=[{"id": lzma.FILTER_LZMA2, "preset": preset, "lc": lc, "lp": lp, "pb": pb, "dict_size": dict_size}])


def main():
    import oracle as O
    out = {"n": np.array(len(VECTORS))}
    for i, (lc, lp, pb, d, preset, recipe) in enumerate(VECTORS):
        x = content(O, recipe)
        c = xz_raw(x, lc, lp, pb, d, preset)
        assert lzma.decompress(c, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": d}]) == x.tobytes()
        out["stream%d" % i] = np.frombuffer(c, dtype=np.uint8)
        out["props%d" % i] = np.array([lc, lp, pb, dict_prop(d)], dtype=np.uint8)
        out["size%d" % i] = np.array(x.size)
        out["sha%d" % i] = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), dtype=np.uint8)
        out["recipe%d" % i] = np.frombuffer(recipe.encode(), dtype=np.uint8)
    path = os.path.join(HERE, "lzma2_xz_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
