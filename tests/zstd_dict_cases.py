"""The cases of tests/test_zstd_dict.py (raw-content zstd dictionaries: include/gpucodec.h "ZSTD, dictionaries"; DESIGN.md section 4 "Dictionaries") and what they share:
the records generator, the reference's dictionary calls, the model of hand-built frames behind a dictionary, and the recorded sizes of tests/golden/zstd_dict_sizes.json.
Backends, batches and the layout check come from tests/zstd_batch_cases.py."""
import ctypes as C
import functools
import importlib.util
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


K = _load("zstd_batch_cases")          # Backend, run_batch, check_layout, text, rand, packed, MATCH_CAP, BLK
Z = _load("zstd_build")                # the frame builder and model (imported, not changed)

BLK, MATCH_CAP = K.BLK, K.MATCH_CAP
GC_OK, GC_ERR_PARAM, GC_ERR_CORRUPT, GC_ERR_UNSUPPORTED = 0, -5, -6, -7
DICT_MAX = 128 << 10
DICT_MAGIC = 0xEC30A437
DICT_SIZES = (8, 9, 63, 64, 65, 1023, 1024, 1025, 16 << 10, DICT_MAX - 1, DICT_MAX)
ITEM_SIZES = (0, 1, 7, 8, MATCH_CAP + 15, MATCH_CAP + 16, MATCH_CAP + 17, 300, 1024, 1025, 4096, BLK)
LEVELS = (1, 3, 12, 19)
REF_LEVELS = (1, 3, 19)
SIZES_PATH = os.path.join(HERE, "golden", "zstd_dict_sizes.json")
MANY_ITEMS, MANY_ROUND_ITEMS, MANY_SPOT, MANY_DICT = 600, 256, 32, 112 << 10


# ------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def _words():
    w = [x for x in K._corpus("text-zipf", 1 << 20).split() if 1 <= len(x) <= 14]
    assert len(w) > 1000
    return w


_LEVELS = (b"DEBUG", b"INFO", b"WARN", b"ERROR")
_SERVICES = (b"auth", b"billing", b"gateway", b"search", b"storage", b"scheduler")
_REGIONS = (b"eu-west-1", b"us-east-2", b"ap-south-1")


@functools.lru_cache(maxsize=None)
def _records(n, seed):
    rng = np.random.default_rng(seed)
    words, out, size = _words(), [], 0
    while size < n:
        msg = b" ".join(words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(3, 41))))
        line = b'{"ts": %d, "level": "%s", "service": "%s", "region": "%s", "request_id": "%08x-%04x", "user": %d, "latency_ms": %d, "status": %d, "message": "%s"}\n' % (
            1700000000 + int(rng.integers(0, 10 ** 7)), _LEVELS[int(rng.integers(0, 4))], _SERVICES[int(rng.integers(0, 6))], _REGIONS[int(rng.integers(0, 3))],
            int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), int(rng.integers(1, 100000)), int(rng.integers(0, 5000)),
            (200, 201, 204, 301, 400, 403, 404, 500, 503)[int(rng.integers(0, 9))], msg)
        out.append(line)
        size += len(line)
    return b"".join(out)[:n]


def records(n, seed):
    """n bytes of JSON-like log lines: fixed field names, random numbers and ids, a few enumerated strings, a message of 3-40 words of text-zipf"""
    return np.frombuffer(_records(n, seed), dtype=np.uint8)


def record_dict(n, seed=1001):
    return records(n, seed)


def record_items(count, size, seed=2002):
    """`count` items of `size` bytes cut from one stream of records (another seed than the dictionary's)"""
    return [records(count * size, seed)[i * size:(i + 1) * size] for i in range(count)]


def text_dict(n):
    return K.text(n, 300000)


def mixed_dict(n):
    """half text-zipf, half records (the records last: nearest to the items)"""
    return np.concatenate([text_dict(n // 2), record_dict(n - n // 2)]) if n >= 16 else text_dict(n)


def sweep_items():
    """the sizes of ITEM_SIZES, alternately records and text"""
    return [(records(n, 3000 + i) if i & 1 else K.text(n, 700 * i)) for i, n in enumerate(ITEM_SIZES)]


def many_batch():
    """GPU only: 600 record items of 300 B .. 4 KiB -> (buffer, items)"""
    rng = np.random.default_rng(601)
    sizes = rng.integers(300, 4097, MANY_ITEMS)
    src = records(int(sizes.sum()), 4004)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return src, [(int(o), int(n)) for o, n in zip(offs, sizes)]


# ------------------------------------------------------------------------------------------------ the reference's dictionary calls
class Ref:
    """ZSTD_compress_usingDict / ZSTD_decompress_usingDict of the reference library (oracle.ref("zstd"))"""
    def __init__(self, lib):
        self.lib = lib
        for name, res, args in (("ZSTD_createCCtx", C.c_void_p, []), ("ZSTD_createDCtx", C.c_void_p, []), ("ZSTD_isError", C.c_uint, [C.c_size_t]),
                                ("ZSTD_compress_usingDict", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]),
                                ("ZSTD_decompress_usingDict", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t])):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        self.cctx, self.dctx = lib.ZSTD_createCCtx(), lib.ZSTD_createDCtx()
        assert self.cctx and self.dctx

    @staticmethod
    def _buf(b):
        a = np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b, dtype=np.uint8)
        return a, (a.ctypes.data if a.size else None)

    def compress(self, data, dictionary, level=3):
        """-> bytes (dictionary None or empty: none)"""
        a, ap = self._buf(data)
        d, dp = self._buf(dictionary if dictionary is not None else b"")
        cap = a.size + (a.size >> 7) + 1024
        out = np.empty(cap, np.uint8)
        r = self.lib.ZSTD_compress_usingDict(self.cctx, out.ctypes.data, cap, ap, a.size, dp, d.size, level)
        assert not self.lib.ZSTD_isError(r)
        return out[:r].tobytes()

    def decompress(self, frame, dictionary, cap):
        """-> numpy content, or None where the reference refuses the frame"""
        a, ap = self._buf(frame)
        d, dp = self._buf(dictionary if dictionary is not None else b"")
        out = np.empty(max(1, cap), np.uint8)
        r = self.lib.ZSTD_decompress_usingDict(self.dctx, out.ctypes.data, cap, ap, a.size, dp, d.size)
        return None if self.lib.ZSTD_isError(r) else out[:r]


# ------------------------------------------------------------------------------------------------ the model
class DictFrame(Z.Frame):
    """zstd_build.Frame behind a raw-content dictionary: `out` starts as the dictionary, so execute()'s `off > len(out)` is the dictionary rule; the content and the
    checksum leave the dictionary out again"""
    def __init__(self, dictionary=b""):
        super().__init__()
        self.dictionary = bytes(dictionary)
        self.out = bytearray(self.dictionary)

    @property
    def content(self):
        return bytes(self.out[len(self.dictionary):])

    def bytes(self, header=None, checksum_value=None, **kw):
        if "fcs" not in kw and header is None:
            kw["fcs"] = len(self.content)
        out = (Z.frame_header(**kw) if header is None else header) + bytes(self.body)
        if kw.get("checksum") or checksum_value is not None:
            out += struct.pack("<I", (Z.xxh64(self.content) & 0xFFFFFFFF) if checksum_value is None else checksum_value)
        return out


def handmade(dictionary):
    """name -> DictFrame built behind `dictionary` (at least 64 bytes; b"" builds the same blocks for the verdict without one).  Every frame is sound WITH the dictionary
    unless its name ends in "_bad"; without one every frame but "no_reach" reaches in front of itself."""
    D = bytes(dictionary)
    n = len(D)
    lits = bytes(range(65, 65 + 40))
    out = {}

    def new():
        return DictFrame(D)

    # first sequence with ll = 0 and offset value 1: repeat offset 2 = 4, the dictionary's fourth byte from the end
    f = new(); f.compressed(Z.lit_raw(lits[:10]), lits[:10], [(0, 6, 1), (4, 5, 4 + 3)], last=True); out["ll0_rep"] = f
    # offset = produced + 3, ml = 100: three bytes of the dictionary, then the frame from its start and over the match's own output
    f = new(); f.compressed(Z.lit_raw(lits[:20]), lits[:20], [(7, 100, 7 + 3 + 3), (5, 4, 2 + 3)], last=True); out["span"] = f
    # exactly produced + dictSize: the dictionary's first byte; one more is damage
    if n:
        f = new(); f.compressed(Z.lit_raw(lits[:12]), lits[:12], [(5, 8, 5 + n + 3), (3, 4, 1)], last=True); out["first_byte"] = f
    f = new(); f.compressed(Z.lit_raw(lits[:12]), lits[:12], [(5, 8, 5 + n + 1 + 3), (3, 4, 1)], last=True); out["past_first_bad"] = f
    # a raw and an RLE block first, then a compressed block whose matches reach the dictionary
    f = new(); f.raw(lits[:30]); f.rle(0x5A, 50)
    f.compressed(Z.lit_raw(lits[:9]), lits[:9], [(2, 20, 80 + 2 + 10 + 3), (3, 70, 80 + 2 + 20 + 3 + 33 + 3), (1, 9, 1)], last=True); out["raw_rle_then"] = f
    # a second compressed block whose symbolic repeat offset reaches the dictionary: block 1 leaves rep = [40, ...]; block 2 starts 30 bytes in with ll = 2 and repeat 1
    f = new(); f.compressed(Z.lit_raw(lits[:24]), lits[:24], [(10, 6, 10 + 30 + 3 - 0)], last=False)
    f.compressed(Z.lit_raw(lits[24:32]), lits[24:32], [(2, 12, 1), (3, 5, 2 + 3)], last=True); out["second_block_rep"] = f
    # no reference in front of the frame at all
    f = new(); f.compressed(Z.lit_raw(lits[:16]), lits[:16], [(8, 12, 5 + 3), (4, 6, 1)], last=True); out["no_reach"] = f
    return out


# ------------------------------------------------------------------------------------------------ coders
def dict_coders(pkg, B, dictionary, level=3):
    enc, dec = pkg.ZstdEncoder(level=level, **B.kw), pkg.ZstdDecoder(**B.kw)
    if dictionary is not None:
        enc.set_dictionary(dictionary)
        dec.set_dictionary(dictionary)
    return enc, dec


def frames_of(out, results):
    return [out[r.dst_off:r.dst_off + r.dst_size].tobytes() for r in results]


def raw_decode(dec, data, cap):
    """gc_zstd_decompress_host as the C ABI has it -> (return code, content)"""
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8))
    out = np.empty(max(1, cap), np.uint8)
    n = C.c_size_t(0)
    rc = dec._lib.gc_zstd_decompress_host(dec._ctx, a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n))
    return rc, out[:n.value]


def raw_set_dictionary(coder, data):
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8))
    coder.dictionary_size()                                      # (declares the prototypes)
    coder._lib.gc_zstd_set_dictionary.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    coder._lib.gc_zstd_set_dictionary.restype = C.c_int
    return coder._lib.gc_zstd_set_dictionary(coder._ctx, a.ctypes.data if a.size else None, a.size)


def last_error(coder):
    return coder._lib.gc_last_error_message(coder._ctx).decode()


# ------------------------------------------------------------------------------------------------ recorded sizes
SIZE_BATCHES = {"records-300": (32, 300), "records-1024": (32, 1024)}      # name -> (items, bytes each); dictionary: 16 KiB of records
SIZE_DICT = 16 << 10


def size_batch(name):
    count, size = SIZE_BATCHES[name]
    return record_dict(SIZE_DICT), record_items(count, size)


def golden_sizes():
    with open(SIZES_PATH) as f:
        return json.load(f)


def sweep_dictionary(ds):
    return mixed_dict(ds)


def sweep_total(pkg, B, ds):
    """-> (dictionary, items, frames, results, total) of the size sweep at dictionary size ds, through the device-pointer batch call"""
    d, parts = sweep_dictionary(ds), sweep_items()
    src, items = K.packed(parts)
    enc = pkg.ZstdEncoder(level=3, **B.kw)
    try:
        enc.set_dictionary(d)
        results, total, out, _ = K.run_batch(B, enc, src, items)
    finally:
        enc.close()
    return d, parts, frames_of(out, results), results, total, items


def measure_sizes(pkg, B, ref=None):
    """what tests/golden/zstd_dict_sizes.json records (tests/golden/make_zstd_dict_sizes.py writes it from the emulator): per size batch the engine's total with and
    without the dictionary and the reference's at level 3; per dictionary size the sweep's total"""
    out = {}
    for name in SIZE_BATCHES:
        d, items = size_batch(name)
        enc = pkg.ZstdEncoder(level=3, **B.kw)
        try:
            e = {"engine_plain": sum(len(f) for f in enc.code_batch(items))}
            enc.set_dictionary(d)
            e["engine_dict"] = sum(len(f) for f in enc.code_batch(items))
        finally:
            enc.close()
        if ref is not None:
            e["ref_plain"] = sum(len(ref.compress(x, None, 3)) for x in items)
            e["ref_dict"] = sum(len(ref.compress(x, d, 3)) for x in items)
        out[name] = e
    out["sweep"] = {str(ds): sweep_total(pkg, B, ds)[4] for ds in DICT_SIZES}
    return out


# ------------------------------------------------------------------------------------------------ walking a frame's sequences (RFC 8878 3.1.1.3.2, the reading side of zstd_build)
class _Fwd:
    def __init__(self, data, pos):
        self.v, self.n = int.from_bytes(data[pos:pos + 512], "little"), 0

    def peek(self, bits):
        return (self.v >> self.n) & ((1 << bits) - 1)

    def read(self, bits):
        r = self.peek(bits)
        self.n += bits
        return r


def read_ncount(data, pos):
    """an FSE table description at data[pos:] -> (norm, log, bytes it takes): the inverse of zstd_build.ncount"""
    r = _Fwd(data, pos)
    log = r.read(4) + 5
    remaining, threshold, nbits, norm = (1 << log) + 1, 1 << log, log + 1, []
    while remaining > 1:
        mx = (2 * threshold - 1) - remaining
        if r.peek(nbits - 1) < mx:
            v = r.read(nbits - 1)
        else:
            v = r.read(nbits)
            if v >= threshold:
                v -= mx
        count = v - 1
        remaining -= abs(count)
        norm.append(count)
        while remaining < threshold and threshold > 1:
            nbits -= 1
            threshold >>= 1
        if count == 0:
            while True:
                rep = r.read(2)
                norm += [0] * rep
                if rep != 3:
                    break
    return norm, log, (r.n + 7) // 8


def walk_sequences(frame):
    """the sequences of every compressed block of one frame -> [(literal length, match length, offset value)] per block (raw / RLE blocks: None)"""
    f = bytes(frame)
    assert struct.unpack("<I", f[:4])[0] == Z.MAGIC
    fhd = f[4]
    single, did, fcs = (fhd >> 5) & 1, (0, 1, 2, 4)[fhd & 3], (0, 2, 4, 8)[fhd >> 6]
    pos = 5 + (0 if single else 1) + did + (fcs if fcs else single)
    blocks = []
    while True:
        h = f[pos] | (f[pos + 1] << 8) | (f[pos + 2] << 16)
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        pos += 3
        if btype != 2:
            blocks.append(None)
            pos += 1 if btype == 1 else size
        else:
            blocks.append(_block_sequences(f[pos:pos + size]))
            pos += size
        if last:
            return blocks


def _block_sequences(b):
    ltype, sf = b[0] & 3, (b[0] >> 2) & 3
    if ltype < 2:
        hdr = (1, 2, 1, 3)[sf]
        regen = int.from_bytes(b[:hdr], "little") >> (3 if hdr == 1 else 4)
        p = hdr + (regen if ltype == 0 else 1)
    else:
        hdr, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        p = hdr + ((int.from_bytes(b[:hdr], "little") >> (4 + bits)) & ((1 << bits) - 1))
    if b[p] < 128:
        n, p = b[p], p + 1
    elif b[p] < 255:
        n, p = ((b[p] - 128) << 8) + b[p + 1], p + 2
    else:
        n, p = b[p + 1] + (b[p + 2] << 8) + 0x7F00, p + 3
    if n == 0:
        return []
    modes = b[p]
    p += 1
    tabs = []
    for w, shift in ((Z.LL, 6), (Z.OF, 4), (Z.ML, 2)):
        m = (modes >> shift) & 3
        if m == Z.MODE_PREDEFINED:
            tabs.append(Z.FseTable(*Z.DEFAULTS[w]))
        elif m == Z.MODE_RLE:
            tabs.append(Z.FseTable.of_rle(b[p]))
            p += 1
        else:
            assert m == Z.MODE_FSE, "a repeated table in a frame of one block"
            norm, log, used = read_ncount(b, p)
            tabs.append(Z.FseTable(norm, log))
            p += used
    v = int.from_bytes(b[p:], "little")
    left = v.bit_length() - 1                                     # (the end mark)

    def read(bits):
        nonlocal left
        left -= bits
        return (v >> left) & ((1 << bits) - 1) if left >= 0 else (v << -left) & ((1 << bits) - 1)

    st = [read(tabs[w].log) for w in (Z.LL, Z.OF, Z.ML)]
    out = []
    for i in range(n):
        llc, ofc, mlc = (tabs[w].sym[st[w]] for w in (Z.LL, Z.OF, Z.ML))
        ofv = (1 << ofc) + read(ofc)
        ml = Z.ML_BASE[mlc] + read(Z.ML_BITS[mlc])
        ll = Z.LL_BASE[llc] + read(Z.LL_BITS[llc])
        out.append((ll, ml, ofv))
        if i + 1 < n:
            for w in (Z.LL, Z.ML, Z.OF):
                st[w] = tabs[w].base[st[w]] + read(tabs[w].nb[st[w]])
    assert left == 0, "the sequences did not use up their bitstream"
    return out


def walk_offsets(frame):
    """-> [(position in the content, match length, offset)] of one frame of one compressed block, the repeat offsets resolved by the model (zstd_build.resolve)"""
    (seqs,) = walk_sequences(frame)
    rep, pos, out = [1, 4, 8], 0, []
    for ll, ml, ofv in seqs:
        off, rep = Z.resolve(rep, ofv, ll)
        pos += ll
        out.append((pos, ml, off))
        pos += ml
    return out
