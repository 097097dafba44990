"""Shared tables and helpers of tests/test_xz.py (the emulator tests and the GPU tests run the same cases): the CRC-64 oracle, the lengths at which the segmented check
kernel changes its path, the encoder's inputs, and an .xz container writer of the TESTS' own (written from the format's description, independent of csrc/gc_xz.h) that
assembles multi-block files from raw LZMA2 streams of Python's `lzma`."""
import lzma
import struct
import zlib

import numpy as np

MiB = 1 << 20
BLK = 128 * 1024

# ---------------------------------------------------------------------------------------------- CRC-64/XZ, table-driven (the oracle of the raw checksum)
_POLY = 0xC96C5795D7870F42
_T = []
for _i in range(256):
    _r = _i
    for _ in range(8):
        _r = (_r >> 1) ^ (_POLY if _r & 1 else 0)
    _T.append(_r)


def crc64_at(data, lengths):
    """{n: CRC-64 of data[:n]} for every n of `lengths` from ONE pass over the bytes (the lengths are prefixes of one another's content)"""
    want = sorted(set(lengths)); out = {}; r = 0xFFFFFFFFFFFFFFFF; k = 0; T = _T
    while k < len(want) and want[k] == 0:
        out[0] = 0; k += 1
    for i, b in enumerate(bytes(data[:want[-1]] if want else b""), 1):
        r = T[(r ^ b) & 0xFF] ^ (r >> 8)
        if i == want[k]:
            out[i] = r ^ 0xFFFFFFFFFFFFFFFF; k += 1
    return out


def crc64(data):
    n = len(bytes(data))
    return crc64_at(data, [n])[n]


# lengths: empty and sub-word; the 4 KiB slice edge; the 1 MiB piece edge; several pieces plus a tail
CRC_LENGTHS = [0, 1, 7, 8, 4095, 4096, 4097, MiB - 1, MiB, MiB + 1, 2 * MiB + 4096 + 3]
CRC_SHIFTS = [0, 1, 3, 15]          # the buffer's first byte against a 16-byte boundary
CRC_FILLS = ["random", "zeros", "ones"]


def fill_bytes(kind, n, seed=5):
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)          # leading zeros: what a design that aligns segments to their END must not get wrong
    if kind == "ones":
        return np.full(n, 0xFF, dtype=np.uint8)
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


_CRC_WANT = {}


def crc64_expected(kind):
    """{length: CRC-64} of fill_bytes(kind, ...)[:length] for every length of CRC_LENGTHS; computed once per process"""
    if kind not in _CRC_WANT:
        _CRC_WANT[kind] = crc64_at(fill_bytes(kind, CRC_LENGTHS[-1]), CRC_LENGTHS)
    return _CRC_WANT[kind]


def segment_plan():
    """About 300 segments back to back from offset 1: every length of CRC_LENGTHS at least once (the four of a MiB and more exactly once, so that the Python oracle stays
    quick), zero-length ones in between.  -> [(offset, length)], the bytes the buffer needs"""
    rng = np.random.default_rng(17)
    small = [n for n in CRC_LENGTHS if n < MiB]
    lens = list(CRC_LENGTHS) + [0] * 25 + [int(small[i]) for i in rng.integers(0, len(small), size=300 - len(CRC_LENGTHS) - 25)]
    order = rng.permutation(len(lens))
    segs = []; off = 1
    for i in order:
        segs.append((off, lens[i])); off += lens[i]
    return segs, off + 16


# ---------------------------------------------------------------------------------------------- encoder cases
ENC_LEVELS = [1, 5, 9]
ENC_CHECKS = ["none", "crc32", "crc64"]
ENC_BLOCK_BYTES = [4096, 65536, 0]
ENC_INPUTS = ["empty", "one", "silesia", "random", "mix"]
CHECK_IDS = {"none": 0, "crc32": 1, "crc64": 4}
LZMA_CHECKS = {"none": lzma.CHECK_NONE, "crc32": lzma.CHECK_CRC32, "crc64": lzma.CHECK_CRC64}


def mix(O, scale=1):
    """text + bytes that do not compress + zeros + text again (test_lzma2_dec._mix): xz writes the chunk kinds 0xE0, 0x80, 0xA0 and 0x02 for it"""
    t = O.corpus("text-zipf", 300_000 * scale)
    return np.concatenate([t, O.corpus("random", 250_000 * scale), np.zeros(400_000 * scale, dtype=np.uint8), t[:300_000 * scale]])


def enc_input(O, name):
    if name == "empty":
        return np.empty(0, dtype=np.uint8)
    if name == "one":
        return np.frombuffer(b"x", dtype=np.uint8).copy()
    if name == "silesia":
        return O.corpus("silesia-like", BLK + 5000)
    if name == "random":
        return O.corpus("random", 300_000)           # raw (stored) chunks
    return mix(O)


def expected_blocks(n, block_bytes):
    return 0 if n == 0 else (1 if block_bytes == 0 else (n + block_bytes - 1) // block_bytes)


# ---------------------------------------------------------------------------------------------- a container writer of the tests' own
def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80); v >>= 7
    out.append(v)
    return bytes(out)


def _crc32(b):
    return struct.pack("<I", zlib.crc32(bytes(b)) & 0xFFFFFFFF)


def dict_prop(size):
    for p in range(40):
        if ((2 | (p & 1)) << (p // 2 + 11)) >= size:
            return p
    return 40


def raw_lzma2(x, dict_size=1 << 20, preset=6, lc=3, lp=0, pb=2):
    return lzma.compress(bytes(x), format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": preset, "lc": lc, "lp": lp, "pb": pb, "dict_size": dict_size}])


def check_bytes(check, content):
    if check == "crc32":
        return _crc32(content)
    if check == "crc64":
        return struct.pack("<Q", crc64(content))
    return b""


def build_stream(parts, check="crc64", filters=None):
    """parts: [(content bytes, dict size, whether the Block Header states the sizes)] -> (the stream's bytes, layout [dict(src_off, src_size, dst_size, check_off, dict_prop)]
    with offsets relative to the stream).  filters: the Block Header's filter list as bytes and their count, instead of LZMA2 alone."""
    flags = bytes([0, CHECK_IDS[check]])
    out = bytearray(b"\xFD7zXZ\x00" + flags + _crc32(flags))
    records = []; layout = []
    for content, dict_size, with_sizes in parts:
        content = bytes(content)
        payload = raw_lzma2(content, dict_size)
        prop = dict_prop(dict_size)
        flt, nflt = filters if filters else (b"\x21\x01" + bytes([prop]), 1)
        body = bytes([(nflt - 1) | (0xC0 if with_sizes else 0)]) + ((vli(len(payload)) + vli(len(content))) if with_sizes else b"") + flt
        size = (1 + len(body) + 3) // 4 * 4 + 4
        hdr = bytes([size // 4 - 1]) + body
        hdr += bytes(size - 4 - len(hdr))
        hdr += _crc32(hdr)
        start = len(out)
        out += hdr + payload + bytes(-len(payload) % 4)
        layout.append(dict(src_off=start + len(hdr), src_size=len(payload), dst_size=len(content), check_off=len(out), dict_prop=prop))
        out += check_bytes(check, content)
        records.append((len(hdr) + len(payload) + len(check_bytes(check, content)), len(content)))
    index = b"\x00" + vli(len(records)) + b"".join(vli(u) + vli(c) for u, c in records)
    index += bytes(-len(index) % 4)
    index += _crc32(index)
    tail = struct.pack("<I", len(index) // 4 - 1) + flags
    out += index + _crc32(tail) + tail + b"YZ"
    return bytes(out), layout


def split_parts(x, n_blocks, dict_sizes=(1 << 16, 1 << 20, 1 << 18), sizes_every=2):
    """x cut into n_blocks parts of uneven size, the dictionary sizes taken in turn, every `sizes_every`-th Block Header without the optional size fields"""
    x = bytes(x); cuts = [len(x) * i // n_blocks + (i % 3 if 0 < i < n_blocks else 0) for i in range(n_blocks + 1)]
    return [(x[cuts[i]:cuts[i + 1]], dict_sizes[i % len(dict_sizes)], i % sizes_every != 1) for i in range(n_blocks)]
