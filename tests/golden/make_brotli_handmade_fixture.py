"""Regenerates tests/golden/brotli_handmade.npz: the hand-built brotli streams of tests/test_brotli_dec_handmade.py (written by tests/brotli_build.py from RFC 7932)
together with what the REFERENCE's decoder (oracle/_ref) makes of each: the content of an accepted stream -- its size and SHA-256, and the bytes themselves up to 4 KiB --
or the fact that it refuses the stream.  A case on which the builder's model and the reference decoder disagree is a mistake in the case: nothing is written then.

    python tests/golden/make_brotli_handmade_fixture.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import oracle as O
    import brotli_build as B
    import test_brotli_dec_handmade as T
    if O.ref("brotli") is None:
        sys.exit("oracle/_ref (reference brotli) is not built")
    cases = T.build_cases(O.ref_brotli_dictionary())
    out = {"n": np.array(len(cases))}
    wrong = []
    for i, c in enumerate(cases):
        stream = np.frombuffer(c.stream, dtype=np.uint8)
        try:
            ref = O.ref_brotli_decompress(stream, c.capacity).tobytes()
        except ValueError:
            ref = None
        if c.accepted:
            if ref is None or ref != c.content:
                wrong.append("%s: the reference decoder %s" % (c.name, "refuses it" if ref is None else "decodes %d bytes, the model %d" % (len(ref), len(c.content))))
                continue
            framed = O.ref_brotlimt_decompress(np.frombuffer(B.frame(c.stream, len(ref)), dtype=np.uint8), len(ref) + 65536).tobytes()
            if framed != ref:
                wrong.append("%s: the reference brotli-mt decoder disagrees on the framed stream" % c.name)
        elif ref is not None:
            wrong.append("%s: the reference decoder accepts it (%d bytes)" % (c.name, len(ref)))
            continue
        out["name%d" % i] = np.frombuffer(c.name.encode(), dtype=np.uint8)
        out["covers%d" % i] = np.frombuffer("\n".join(c.covers).encode(), dtype=np.uint8)
        out["stream%d" % i] = stream
        out["flags%d" % i] = np.array([c.accepted, c.needs_dictionary, c.small_lds, c.error or 0, c.capacity, len(ref) if c.accepted else 0], dtype=np.int64)
        if c.accepted:
            out["sha%d" % i] = np.frombuffer(hashlib.sha256(ref).digest(), dtype=np.uint8)
            if len(ref) <= 4096:
                out["content%d" % i] = np.frombuffer(ref, dtype=np.uint8)
    if wrong:
        sys.exit("\n".join(wrong))
    path = os.path.join(HERE, "brotli_handmade.npz")
    np.savez_compressed(path, **out)
    print(path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
