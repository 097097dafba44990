"""Shared by tests/test_emu_pipeline.py (emulator) and tests/test_gpu_parity.py (device): a context's buffers grow with the largest input it has seen, and growing them
must never change a byte.  One encoder per codec takes a small input (one block: the block-local finder), a large one (3 blocks + 12 345 bytes: the per-block workspace
and every array of the finder grow) and the small one again (nothing shrinks, the larger buffers are reused); every output must be what a FRESH encoder makes of the
same input.  The levels are the ones whose parse is the price-based one, so that every finder array is in play."""
import numpy as np

BLK = 128 * 1024
CODECS = {"zstd": ("ZstdEncoder", 5), "flzma2": ("Flzma2Encoder", 5), "brotli": ("BrotliEncoder", 6)}


def inputs(O):
    small, large = O.corpus("text-zipf", 1000), O.corpus("silesia-like", 3 * BLK + 12345)
    return [("small", small), ("large", large), ("small again", small)]


def check_growth_keeps_bytes(pkg, O, codec, **kw):
    """-> {"small": stream, "large": stream} of the reused encoder (equal to the fresh encoders' by then)"""
    cls, level = getattr(pkg, CODECS[codec][0]), CODECS[codec][1]
    fresh, out = {}, {}
    enc = cls(level=level, **kw)
    try:
        for name, x in inputs(O):
            key = name.split()[0]
            if key not in fresh:
                one = cls(level=level, **kw)
                try:
                    fresh[key] = one.code(x).copy()
                finally:
                    one.close()
            got = enc.code(x)
            assert np.array_equal(got, fresh[key]), "%s, %s input (%d bytes): %d bytes from the reused encoder, %d from a fresh one" % (codec, name, x.size, got.size, fresh[key].size)
            out[key] = got.copy()
    finally:
        enc.close()
    return out
