"""Regenerates tests/golden/zstd_handmade.npz: the hand-built zstd frames of tests/test_zstd_dec_handmade.py (written by tests/zstd_build.py from RFC 8878) together with what
the REFERENCE's decoder (oracle/_ref) makes of each: the content of an accepted stream -- its size and SHA-256, and the bytes themselves up to 4 KiB -- or the fact that it
refuses the stream.  A case on which the builder's model and the reference decoder disagree is a mistake in the case: nothing is written then.  The only streams the reference
may accept and this decoder refuses are the ones the test module lists as stricter than the reference.

    python tests/golden/make_zstd_handmade_fixture.py
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
    import test_zstd_dec_handmade as T
    if O.ref("zstd") is None:
        sys.exit("oracle/_ref (reference zstd) is not built")
    cases = T.build_cases()
    names, covers, streams, flags, shas, contents, content_sizes = [], [], [], [], [], [], []
    wrong = []
    for c in cases:
        stream = np.frombuffer(c.stream, dtype=np.uint8)
        try:
            ref = O.ref_zstd_decompress(stream, c.capacity).tobytes()
        except ValueError:
            ref = None
        if c.accepted:
            if ref is None or ref != c.content:
                wrong.append("%s: the reference decoder %s" % (c.name, "refuses it" if ref is None else "decodes %d bytes, the model %d" % (len(ref), len(c.content))))
                continue
        elif (ref is not None) != c.stricter:
            wrong.append("%s: the reference decoder %s" % (c.name, "accepts it (%d bytes)" % len(ref) if ref is not None else "refuses it as well: not a stricter case"))
            continue
        names.append(c.name)
        covers.append("\n".join(c.covers))
        streams.append(c.stream)
        flags.append([c.accepted, c.matches, c.stricter, c.error, c.capacity, len(ref) if c.accepted else 0])
        shas.append(hashlib.sha256(ref).digest() if c.accepted else bytes(32))
        keep = c.accepted and len(ref) <= 4096
        contents.append(ref if keep else b"")
        content_sizes.append(len(ref) if keep else -1)
    if wrong:
        sys.exit("\n".join(wrong))
    path = os.path.join(HERE, "zstd_handmade.npz")
    u8 = lambda data: np.frombuffer(data, dtype=np.uint8)
    np.savez_compressed(path, names=u8("\0".join(names).encode()), covers=u8("\0".join(covers).encode()), streams=u8(b"".join(streams)),
                        stream_sizes=np.array([len(x) for x in streams], dtype=np.int64), flags=np.array(flags, dtype=np.int64), shas=u8(b"".join(shas)).reshape(-1, 32),
                        contents=u8(b"".join(contents)), content_sizes=np.array(content_sizes, dtype=np.int64))
    print(path, len(cases), "cases: the model and the reference decoder agree on all;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
