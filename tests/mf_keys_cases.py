"""The cases of tests/test_mf_keys.py, shared with tools/record_mf_keys.py (which records their stream hashes at another commit), and the numpy model of the finder's
listing predicate and keys (csrc/gc_lz_window.hip mf_list / mf_listed / mf_window / mf_keys) that the test holds the lists of W1..W3 against.

Every input is built for frames of two blocks (test hook GC_FRAME_BLOCKS=2), so that frame starts and ends occur in inputs of at most five blocks.  The bytes are random
literals mixed with copies of earlier bytes (so that positions have candidates everywhere and a position listed or dropped by mistake moves the parse), with planted
structure on top:
  * runs      byte runs of 8..12 bytes starting at every offset mod 4: in the middle of a tile, across tile edges of both geometries (the byte in front of a tile's
              first position comes from the staging pad), across block edges, across a frame edge and at a frame's first byte (which is never inside a run);
  * end+K     K bytes behind a whole frame: the last listed position (frame end - 80) lies at tile offset K - 80 -- 0, 1, 3, 4, 63, 64, or in the tile in front
              (K = tile + 79); K = 79: a second frame in which nothing is listed;
  * tail+K    a last tile of K bytes (lengths not divisible by 4 or 64);
  * short40   a second frame of 40 bytes."""
import hashlib

import numpy as np

BLK = 128 * 1024
FRAME_BLOCKS = 2                # GC_FRAME_BLOCKS of every case
FRAME = FRAME_BLOCKS * BLK
WINDOW = 64 + 16                # GC_MATCH_CAP + 16: a listed position has this many bytes left in its frame

# (codec, level, tile bytes of the geometry the level runs): zstd 3 = base keys, fast; zstd 5 = far, far2 and short passes on the fast geometry; the other two = wide
CODECS = (("zstd", 3, 8192), ("zstd", 5, 8192), ("flzma2", 5, 16384), ("zstd", 19, 16384))
END_KS = (79, 80, 81, 83, 84, 143, 144)
TAIL_KS = (1, 2, 3, 5, 63, 65)


def _base(n, seed):
    rng = np.random.RandomState(seed)
    out = np.empty(n + 64, np.uint8)
    i = 0
    while i < n:
        if i > 64 and rng.randint(3):                   # two in three: a copy of 8..40 bytes from at most 64 KiB back
            ln = rng.randint(8, 41)
            d = rng.randint(ln, min(i, 65536) + 1)
            out[i:i + ln] = out[i - d:i - d + ln]
        else:
            ln = rng.randint(4, 21)
            out[i:i + ln] = rng.randint(0, 256, ln)
        i += ln
    return out[:n].copy()


def _plant_run(x, pos, length):
    """x[pos : pos + length] = one byte value that differs from both neighbours: a run of exactly `length` bytes"""
    if pos < 0 or pos + length > x.size:
        return
    b = 0
    while (pos > 0 and x[pos - 1] == b) or (pos + length < x.size and x[pos + length] == b):
        b += 1
    x[pos:pos + length] = b


def _periodic(x, start, seed):
    """x[start:] = random bytes of period 37: every position from start + 37 on has a candidate 37 bytes back"""
    if start < x.size:
        p = np.random.RandomState(seed).randint(0, 256, 37).astype(np.uint8)
        x[start:] = np.resize(p, x.size - start)


def _runs_input(tile):
    n = 2 * FRAME + 12345
    x = _base(n, 11)
    for k in range(20):                                  # mid-tile: every start offset mod 4 with every length 8..12
        _plant_run(x, 3 * tile + 1000 + 64 * k + k % 4, 8 + k // 4)
    edges = [8192 * m for m in range(1, 16)] + [FRAME + 8192 * m for m in range(1, 9)] + [BLK, 3 * BLK, 4 * BLK]
    for k, e in enumerate(edges):                        # across tile and block edges: the run starts 0..11 bytes in front of the edge
        _plant_run(x, e - k % 12, 8 + k % 5)
    _plant_run(x, 0, 12)                                 # the input's first byte
    _plant_run(x, FRAME - 4, 12)                         # across a frame edge: the frame's first byte continues the run in front of it, and is listed
    _plant_run(x, 2 * FRAME, 12)                         # from a frame's first byte on
    _plant_run(x, 2 * FRAME + tile - 3, 11)
    return x


def _end_input(k, seed):
    x = _base(FRAME + k, seed)
    _periodic(x, max(FRAME, x.size - 400), seed + 1)
    x[FRAME - 400:FRAME] = np.resize(np.random.RandomState(seed + 2).randint(0, 256, 41).astype(np.uint8), 400)      # the first frame's end likewise (period 41)
    return x


def build(name, tile):
    """the input of case `name` for a geometry with tiles of `tile` bytes"""
    if name == "runs":
        return _runs_input(tile)
    if name.startswith("end+"):
        return _end_input(int(name[4:]), 100)
    if name.startswith("endtile+"):
        return _end_input(tile + int(name[8:]), 200)
    if name.startswith("tail+"):
        x = _base(FRAME + tile + int(name[5:]), 300)
        _plant_run(x, x.size - 9, 9)
        return x
    if name == "short40":
        return _end_input(40, 400)
    raise KeyError(name)


NAMES = ("runs",) + tuple("end+%d" % k for k in END_KS) + tuple("endtile+%d" % k for k in END_KS) + tuple("tail+%d" % k for k in TAIL_KS) + ("short40",)
# what the lists themselves are checked on (tests/test_mf_keys.py test_lists_match_model): every input -- a wrong list limit shows at the frame-end offsets and
# the odd tails, and there the model names W1 or W3
MODEL_NAMES = NAMES


def cases():
    """(codec, level, tile, name) of every stream case; the emulator and the device run the same ones"""
    return [(codec, level, tile, name) for codec, level, tile in CODECS for name in NAMES]


def case_id(case):
    return "%s-%d/%s" % (case[0], case[1], case[3])


def stream_sha256(pkg, case, **enc_kw):
    """Compress the case's input with a fresh encoder (lib_path=<a test build> [+ device=<n>]; GC_FRAME_BLOCKS is the caller's to set) and hash the stream."""
    codec, level, tile, name = case
    cls = {"zstd": pkg.ZstdEncoder, "flzma2": pkg.Flzma2Encoder}[codec]
    enc = cls(level=level, **enc_kw)
    try:
        c = enc.code(build(name, tile))
    finally:
        enc.close()
    return hashlib.sha256(np.ascontiguousarray(c, dtype=np.uint8).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------- the model
MODE_BASE, MODE_FAR = 0, 1


def _u32(x, off, idx):
    """little-endian 32-bit words at x[idx + off] (x padded with zeros), as uint64 for arithmetic mod 2^32"""
    b = [x[idx + off + i].astype(np.uint64) for i in range(4)]
    return b[0] | (b[1] << np.uint64(8)) | (b[2] << np.uint64(16)) | (b[3] << np.uint64(24))


def model_lists(data, fast, mode, frame_blocks=FRAME_BLOCKS):
    """What W1..W3 must leave for `data`: (counts [frame][tile][partition], entries per frame: a uint64 array in (partition, position) order)."""
    M = np.uint64(0xFFFFFFFF)
    def mul(a, k): return (a * np.uint64(k)) & M
    def sh(a, s): return a >> np.uint64(s)
    tile, part_log, pos_bits = (8192, 8, 23) if fast else (16384, 10, 24)
    frame = frame_blocks * BLK
    n = data.size
    x = np.concatenate([np.asarray(data, np.uint8), np.zeros(64, np.uint8)])
    counts, entries = [], []
    for fs in range(0, ((n + BLK - 1) // BLK + frame_blocks - 1) // frame_blocks * frame, frame):
        fe = min(fs + frame, n)
        P = np.arange(fs, max(fs, fe - WINDOW + 1), dtype=np.int64)                 # positions with a full window left in the frame
        same = np.ones(P.size, bool)
        for i in range(8):
            same &= x[P + i] == x[np.maximum(P - 1, 0) + i]
        P = P[~(same & (P > fs))]
        lo, hi = _u32(x, 0, P), _u32(x, 4, P)
        hL = (mul(lo, 0x9E3779B1) + mul(hi, 0x85EBCA77)) & M
        hS = (mul(lo, 0x9E3779B1) + mul(hi & np.uint64(0xFF), 0xC2B2AE3D)) & M
        if mode == MODE_FAR:
            hS = (hL + mul(_u32(x, 8, P), 0xC2B2AE3D)) & M
            hS ^= sh(hS, 15); hS = mul(hS, 0x2C1B3C6D)
            hL = (hS + mul(_u32(x, 12, P), 0x27D4EB2F)) & M
            hL ^= sh(hL, 13); hL = mul(hL, 0x165667B1)
        part = sh(hS, 32 - part_log).astype(np.int64)
        kL, kS = sh(hL, 12), sh(hS, 32 - part_log - 19) & np.uint64((1 << 19) - 1)
        ent = (P - fs).astype(np.uint64) | (kL << np.uint64(pos_bits)) | (kS << np.uint64(pos_bits + 20))
        order = np.argsort(part, kind="stable")
        entries.append(ent[order])
        tpf = frame // tile
        counts.append(np.bincount((P - fs) // tile * (1 << part_log) + part, minlength=tpf << part_log).reshape(tpf, 1 << part_log))
    return np.array(counts), entries
