"""The cases of tests/test_xxh64.py and tests/test_zstd_checksum.py and the checks both sides share: the emulator and the device run the same ones.

XXH64 (gc_xxh64_device against the oracle's gco_xxh64):
  * every branch of the finalisation -- below 32 bytes and from 32 up, the 8-, 4- and 1-byte tails: 0 1 3 4 7 8 31 32 33 47 63 64 95;
  * the edges of the kernel's staging tile T (GC_XXH64_TILE of csrc/gc_common.h): T - 1, T, T + 1 and 2 T + 13 (a whole tile, a second one, a part of a third);
  * a buffer of 3 T + 45 bytes that starts 1, 4 and 7 bytes behind an aligned allocation.

Content checksums (GC_OPT_ZSTD_CHECKSUM): levels 1, 3 and 19 on text at the sizes below under 256 KiB frames (test hook GC_FRAME_BLOCKS=2) -- empty, below and at one
stripe, one block (the block-local finder), one frame, one frame + 1, a short last frame, four whole frames --, random bytes (raw blocks end every frame), and one
input under the levels' own 8 MiB frames."""
import functools
import struct

import numpy as np

BLK = 128 * 1024
T = 8192                        # the kernel's staging tile in bytes
XXH_SEEDS = (0, 0x9E3779B185EBCA87)
XXH_LENGTHS = (0, 1, 3, 4, 7, 8, 31, 32, 33, 47, 63, 64, 95, T - 1, T, T + 1, 2 * T + 13)
XXH_OFFSET_LEN = 3 * T + 45
XXH_OFFSETS = (1, 4, 7)
XXH_KNOWN = ((b"", 0xEF46DB3751D8E999), (b"abc", 0x44BC2CF5AD770999))

HOOK_FRAME_BLOCKS = 2           # GC_FRAME_BLOCKS of the hooked cases: 256 KiB frames
LEVELS = (1, 3, 19)
SIZES = (0, 5, 31, 32, BLK, 2 * BLK, 2 * BLK + 1, 3 * BLK + 77, 4 * 2 * BLK)
DAMAGE_CASE = (3, "text-zipf", 3 * BLK + 77, True)      # two frames: the second one's checksum gets a bit flipped
PARITY_CASES = ((1, "text-zipf", 2 * BLK + 1, True), (3, "random", 3 * BLK + 77, True), (19, "text-zipf", 4 * 2 * BLK, True))    # device bytes == emulator bytes


def stream_cases():
    """(level, corpus kind, bytes, hooked) of every case that needs no large input"""
    out = [(level, "text-zipf", n, True) for level in LEVELS for n in SIZES]
    out.append((3, "random", 3 * BLK + 77, True))
    return out


def case_id(case):
    return "L%d/%s/%d/%s" % (case[0], case[1], case[2], "hook" if case[3] else "plain")


@functools.lru_cache(maxsize=None)
def _input_bytes(kind, n):
    if kind == "random":
        return np.random.default_rng(20261017).integers(0, 256, n, dtype=np.uint8).tobytes()
    import oracle
    return oracle.corpus(kind, n).tobytes()


def case_input(case):
    return np.frombuffer(_input_bytes(case[1], case[2]), dtype=np.uint8)


def xxh64_input(n):
    return np.frombuffer(_input_bytes("random", XXH_OFFSET_LEN + 64)[:n], dtype=np.uint8)


def frame_bytes(case):
    return (HOOK_FRAME_BLOCKS if case[3] else 64) * BLK


def n_frames(case):
    return max(1, -(-case[2] // frame_bytes(case)))


def _xxh32(O, a):
    a = np.ascontiguousarray(a)
    return O.port().gco_xxh64(a.ctypes.data if a.size else None, a.size, 0) & 0xFFFFFFFF


def encode_all(enc, x):
    """{name: stream} of one input under one encoder: plain, with checksums, with both options, plain again; and the bound"""
    out = {"plain": enc.code(x).copy()}
    enc.set_option(enc.OPT_ZSTD_CHECKSUM, 1)
    out["sum"] = enc.code(x).copy()
    enc.set_option(enc.OPT_ZSTD_SEEK_TABLE, 1)
    out["both"] = enc.code(x).copy()
    enc.set_option(enc.OPT_ZSTD_SEEK_TABLE, 0)
    enc.set_option(enc.OPT_ZSTD_CHECKSUM, 0)
    out["off"] = enc.code(x).copy()
    out["bound"] = enc.compress_bound(x.size)
    return out


def decodes_everywhere(O, dec, c, x):
    """the stream regenerates x under the reference's decoder, the oracle's restatement (refuses a wrong checksum) and the engine's decoder (verifies on the device)"""
    assert np.array_equal(O.ref_zstd_decompress(c, x.size), x)
    assert np.array_equal(O.port_zstd_decompress(c, x.size), x)
    assert np.array_equal(dec.code(c), x)


def walk_checksummed(O, dec, c, x, frames_expected):
    """every frame of c: magic, Content_Checksum_Flag, trailing low 32 bits of XXH64 of its content; -> [(src_off, src_size, checksum)]"""
    frames, nf, total = dec.scan(c)
    assert nf == frames_expected and total == x.size
    b = c.tobytes()
    out, pos = [], 0
    for i in range(nf):
        f = frames[i]
        assert b[f.src_off:f.src_off + 4] == b"\x28\xB5\x2F\xFD"
        assert b[f.src_off + 4] & 4 and f.flags & 1
        end = f.src_off + f.src_size
        have = struct.unpack("<I", b[end - 4:end])[0]
        assert have == _xxh32(O, x[pos:pos + f.content_size]), (i, hex(have))
        out.append((f.src_off, f.src_size, have))
        pos += f.content_size
    assert pos == x.size
    return out


def strip_checksums(c, walked):
    """c without the frames' trailing checksums and flag bits (and without whatever follows the last frame)"""
    b = c.tobytes()
    parts = []
    for off, size, _ in walked:
        fr = bytearray(b[off:off + size - 4])
        fr[4] &= 0xFB
        parts.append(bytes(fr))
    return np.frombuffer(b"".join(parts), dtype=np.uint8)


def check_seek_table(c, walked, x_size, frame_len):
    """the seek table behind the frames: descriptor 0x80, entries { compressed size, decompressed size, checksum } that add up"""
    b = c.tobytes()
    nf = len(walked)
    assert struct.unpack("<I", b[-4:])[0] == 0x8F92EAB1 and b[-5] == 0x80
    assert struct.unpack("<I", b[-9:-5])[0] == nf
    t0 = len(b) - 9 - 12 * nf - 8
    magic, size = struct.unpack("<II", b[t0:t0 + 8])
    assert magic == 0x184D2A5E and size == 12 * nf + 9
    off = dec = 0
    for i, (foff, fsize, fsum) in enumerate(walked):
        cs, ds, xs = struct.unpack("<III", b[t0 + 8 + 12 * i:t0 + 20 + 12 * i])
        assert (off, cs, xs) == (foff, fsize, fsum)
        assert ds == min(frame_len, x_size - dec)
        off += cs; dec += ds
    assert off == t0 and dec == x_size


def check_case(O, dec, case, streams):
    """everything the issue asks of one case"""
    x = case_input(case)
    nf = n_frames(case)
    plain, c, both = streams["plain"], streams["sum"], streams["both"]
    assert np.array_equal(streams["off"], plain)                          # the option set back: the bytes from before it was set
    assert c[:4].tobytes() == b"\x28\xB5\x2F\xFD"
    decodes_everywhere(O, dec, c, x)
    walked = walk_checksummed(O, dec, c, x, nf)
    assert c.size == plain.size + 4 * nf
    assert np.array_equal(strip_checksums(c, walked), plain)
    decodes_everywhere(O, dec, both, x)                                    # (every decoder skips the skippable frame)
    walked2 = walk_checksummed(O, dec, both, x, nf)
    assert walked2 == walked and np.array_equal(both[:c.size], c)          # the table is appended, nothing else changes
    check_seek_table(both, walked2, x.size, frame_bytes(case))
    assert c.size <= streams["bound"] and both.size <= streams["bound"]
