"""Hand-built zstd frames for the device decoder (`gc_zstd_dec.hip`): what RFC 8878 allows and the reference's encoder never writes.  tests/zstd_build.py writes the frames from
the RFC and models the content; tests/golden/zstd_handmade.npz pins every stream together with what the REFERENCE's decoder made of it (content, or its refusal).  Every
accepted stream must decode to the same bytes under the model, the reference decoder and this decoder; every refused stream -- one per check the decoder makes by name -- must
be refused by the reference and by this decoder with the decoder's own error class, leave the output buffer alone and leave the context usable.

CPU: the kernels under the SIMT emulator -- default settings and the four forced combinations of execution path (GC_ZD_WIDE) and sequences kernel (GC_ZD_SEQV).  GPU: the
product library at its own choice of path, the hooks library for the forced combinations.  `python tests/golden/make_zstd_handmade_fixture.py` regenerates the fixture.

What cannot exist and is therefore not an item: literal-length code 35 and match-length code 52 with ALL extra bits set (65536 + 65535 literals and a match of at least 3, or a
match of 65539 + 65535, are more than a block may hold: the largest values that fit stand in); repeat offset "the first minus 1" as the very first sequence of a frame (it is
0: a refused case).  Where the reference decided otherwise than expected: it decodes compressed literals that regenerate 0 bytes (an accepted case here, the decoder follows);
it refuses a nonzero dictionary id and an offset code of 31 as well (plain refused cases of class GC_ERR_PARAM); and its one-pass decoder lets a raw block and a block content
above 128 KiB pass, which RFC 8878 forbids: STRICTER_THAN_THE_REFERENCE names these two, the only streams the reference decodes and this decoder refuses.
One stream stays out on purpose: FSE-coded weights whose last state reads no bits never over-read the stream, so a decoder without a guard on the number of weights would not
return (the builder refuses to write it)."""
import ctypes as C
import hashlib
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_build as Z
from zstd_build import LL, ML, OF, Frame, Huffman, dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "zstd_handmade.npz")
GC_ERR_PARAM, GC_ERR_DST_SMALL, GC_ERR_CORRUPT = -5, -4, -6
PRE, RLE, FSE, REP = Z.MODE_PREDEFINED, Z.MODE_RLE, Z.MODE_FSE, Z.MODE_REPEAT
KIND = {PRE: "predefined", RLE: "RLE", FSE: "FSE"}
TABLE = {LL: "literal lengths", OF: "offsets", ML: "match lengths"}
W128 = 7 << 3                                                     # window descriptor: 128 KiB
BLOCK_MAX = Z.BLOCK_MAX

# ---------------------------------------------------------------------------------------------- what has to be covered, by name
ITEMS_ACCEPTED = (
    ["frame: content size field of %s" % s for s in ("0 bytes", "1 byte", "2 bytes holding 256", "2 bytes holding 65791", "4 bytes", "8 bytes")] +
    ["frame: window descriptor %s" % s for s in ("exponent 0 mantissa 0", "exponent 0 mantissa 7", "exponent 21")] +
    ["frame: dictionary id field of %d bytes holding 0" % n for n in (1, 2, 4)] +
    ["frame: checksum over %d bytes" % n for n in (0, 1, 3, 4, 7, 8, 31, 32, 33)] +
    ["frame: one empty raw last block", "frame: skippable frames of size 0 with every magic nibble between frames"] +
    ["blocks: an empty raw block that is not last"] + ["blocks: %s block of %d bytes" % (k, n) for k in ("raw", "RLE") for n in (1, 131072)] +
    ["blocks: a compressed block of exactly 131072 bytes", "blocks: raw and RLE blocks between compressed blocks keep the repeat offsets, the tree and the tables",
     "blocks: a block of 0 sequences between two with sequences is skipped by Repeat_Mode and the repeat offsets"] +
    ["%s literals: header of %d bytes" % (k, n) for k in ("raw", "RLE") for n in (1, 2, 3)] +
    ["%s literals: %s" % (k, s) for k in ("raw", "RLE") for s in ("size 5 in the 2-byte and the 3-byte form", "size format 10 of the 1-byte form")] +
    ["%s literals: size %d" % (k, n) for k in ("raw", "RLE") for n in (0, 31, 32, 4095, 4096)] +
    ["compressed literals: size format %d" % n for n in range(4)] + ["compressed literals: one stream of %d bytes" % n for n in (0, 1, 1023)] +
    ["compressed literals: four streams of %d bytes" % n for n in (6, 7, 8, 9, 1023)] +
    ["compressed literals: streams of one byte"] + ["compressed literals: end mark in bit %d" % b for b in range(8)] +
    ["tree: direct weights for 2 symbols", "tree: 128 direct weights", "tree: FSE weights, accuracy log 5", "tree: FSE weights, accuracy log 6", "tree: FSE weights, a less-than-one count",
     "tree: FSE weights, zero-run flags 3 + 3 + k", "tree: FSE weights, an odd number", "tree: FSE weights, an even number", "tree: depth 11"] +
    ["tree: all codes of %d bits" % n for n in (1, 2, 4, 7)] + ["tree: all 256 symbols, the implied last weight is symbol 255"] +
    ["treeless: %s" % s for s in ("directly behind the tree", "behind a raw block", "behind a compressed block with raw literals", "two in a row", "one stream", "four streams")] +
    ["sequence count: %s" % s for s in ("1", "127", "128", "0x7EFF", "0x7F00", "0 in the 2-byte form", "5 in the 2-byte form")] +
    ["modes: every combination of predefined, RLE and FSE over the three tables"] +
    ["modes: %s repeated from a %s table" % (TABLE[w], KIND[m]) for w in (LL, OF, ML) for m in (PRE, RLE, FSE)] +
    ["modes: a repeat chained over three blocks", "modes: a source two blocks back behind a raw block and a block of 0 sequences"] +
    ["fse: accuracy log 5", "fse: literal lengths at accuracy log 9", "fse: offsets at accuracy log 8", "fse: match lengths at accuracy log 9", "fse: less-than-one counts and zero runs",
     "fse: two symbols only", "fse: the highest symbols 35, 30 and 52"] +
    ["values: every literal-length code with its extra bits all 0 and all 1", "values: every match-length code with its extra bits all 0 and all 1",
     "values: offset codes 0 to 20 with their extra bits all 0 and all 1"] +
    ["repeat offsets, first sequence of a frame: value %d %s literals" % (v, k) for v, k in ((1, "with"), (2, "with"), (3, "with"), (1, "without"), (2, "without"))] +
    ["repeat offsets, first sequence of a later block: value %d %s literals" % (v, k) for v in (1, 2, 3) for k in ("with", "without")] +
    ["repeat offsets: a symbolic offset decremented three times"] +
    ["shapes: %s" % s for s in ("the last sequence ends the block", "literals behind the last sequence", "ll 0 ml 3", "one match of 131072 bytes at offset 1")] +
    ["bitstream: %d bytes" % n for n in (1023, 1024, 1025, 1032, 2049)] + ["bitstream: end mark in bit %d" % b for b in range(8)] +
    ["geometry: seeded random sequences over three blocks"])
STRICTER_THAN_THE_REFERENCE = ("a raw block above 128 KiB", "block content above 128 KiB")            # the only streams the reference decodes and this decoder refuses


class Case:
    def __init__(self, name, covers, stream, content=None, capacity=None, error=None, matches=False, stricter=False):
        self.name, self.covers, self.stream, self.content = name, [covers] if isinstance(covers, str) else list(covers), bytes(stream), None if content is None else bytes(content)
        self.accepted = error is None
        self.error = error or 0                                   # the error class of a refused stream
        self.capacity = capacity if capacity is not None else (max(len(content), 1) if content is not None else 4096)
        self.matches, self.stricter = matches, stricter


SEED = bytes((i * 37 + 11) & 255 for i in range(300))


def _pattern(n, k=0):
    return bytes(((i * 7 + k) ^ (i >> 5)) & 255 for i in range(n))


def fb(f, **kw):
    """the frame's bytes: a 128 KiB window and a 4-byte content size unless told otherwise"""
    kw.setdefault("fcs", len(f.out))
    if kw["fcs"] is not None and not kw.get("single"):
        kw.setdefault("fcs_bytes", 4)
    if not kw.get("single"):
        kw.setdefault("window", W128)
    return f.bytes(**kw)


def _acc(name, covers, frames, matches=True, **kw):
    """one accepted case of one frame or several"""
    frames = frames if isinstance(frames, list) else [frames]
    assert all(f.sound for f in frames), name
    return Case(name, covers, b"".join(fb(f, **kw) for f in frames), content=b"".join(bytes(f.out) for f in frames), matches=matches)


def _seeded(n=64):
    f = Frame()
    f.raw(SEED[:n])
    return f


# ---------------------------------------------------------------------------------------------- accepted streams
def _frames():
    out = []
    for what, n, kw in (("0 bytes", 10, dict(fcs=None)), ("1 byte", 10, dict(single=True, fcs_bytes=1)), ("2 bytes holding 256", 256, dict(fcs_bytes=2)),
                        ("2 bytes holding 65791", 65791, dict(fcs_bytes=2)), ("4 bytes", 10, dict(fcs_bytes=4)), ("8 bytes", 10, dict(fcs_bytes=8))):
        f = Frame()
        if n > 300:
            f.rle(0x5A, n, last=True)
        else:
            f.raw(_pattern(n), last=True)
        c = Case("fcs_%s" % what.replace(" ", "_"), "frame: content size field of " + what, fb(f, **kw), content=f.out, capacity=n + 7)
        out.append(c)
    for what, byte in (("exponent 0 mantissa 0", 0), ("exponent 0 mantissa 7", 7), ("exponent 21", 21 << 3)):
        f = _seeded(100)
        f.compressed(Z.lit_raw(b"win"), b"win", [(3, 9, 50 + 3)], last=True)
        out.append(Case("window_%02x" % byte, "frame: window descriptor " + what, fb(f, fcs=None, window=byte), content=f.out, capacity=4096, matches=True))
    for n in (1, 2, 4):
        f = Frame()
        f.raw(b"dictionary id 0", last=True)
        out.append(_acc("did_%d_bytes" % n, "frame: dictionary id field of %d bytes holding 0" % n, f, matches=False, did_bytes=n, did=0))
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33):
        f = Frame()
        f.raw(_pattern(n, n), last=True)
        out.append(_acc("checksum_%d" % n, "frame: checksum over %d bytes" % n, f, matches=False, checksum=True))
    f = Frame()
    f.raw(b"", last=True)
    out.append(Case("empty_frame", "frame: one empty raw last block", fb(f, fcs=None), content=b"", capacity=16))
    frames, stream = [], b""
    for nib in range(16):
        f = Frame()
        f.raw(b"frame %02d;" % nib, last=True)
        frames.append(f)
        stream += Z.skippable(nib) + fb(f)
    out.append(Case("skippable_nibbles", "frame: skippable frames of size 0 with every magic nibble between frames", stream + Z.skippable(5), content=b"".join(bytes(f.out) for f in frames)))
    return out


H5 = Huffman([3, 1, 1, 1, 1])                                     # codes of 1 and 3 bits over the symbols 0..4
FSE_LL, FSE_OF, FSE_ML = (dist(36, {0: 8, 2: 16, 5: 8}), 5), (dist(4, {1: 8, 2: 16, 3: 8}), 5), (dist(53, {0: 8, 1: 16, 6: 8}), 5)
FSE_SPEC = {LL: FSE_LL, OF: FSE_OF, ML: FSE_ML}


def _spread(n, codes, log=5):
    """a distribution over n symbols that gives the listed codes all of 1 << log between them"""
    codes = sorted(set(codes))
    share = (1 << log) // len(codes)
    d = dist(n, {c: share for c in codes})
    d[codes[0]] += (1 << log) - share * len(codes)
    return d, log


def _h5(n, k=0):
    return bytes((0, 0, 1, 0, 2, 3, 0, 4)[(i * 5 + k + i // 9) % 8] for i in range(n))


def _mode_block(f, modes, last=False, k=0, lit=None):
    """three sequences whose codes every kind of table here holds: RLE tables allow one code only (ll 2, offset value 4 + x, ml 4)"""
    seqs = []
    for i in range(3):
        ll = 2 if modes[LL] == RLE or f.tables[LL] is not None and f.tables[LL].rle and modes[LL] == REP else (2, 5, 0)[i]
        rle_of = modes[OF] == RLE or f.tables[OF] is not None and f.tables[OF].rle and modes[OF] == REP
        ofv = 4 + (0, 3, 1)[(i + k) % 3] if rle_of else (5, 9, 2)[i]
        ml = 4 if modes[ML] == RLE or f.tables[ML] is not None and f.tables[ML].rle and modes[ML] == REP else (4, 9, 3)[i]
        seqs.append((ll, ml, ofv))
    n = sum(s[0] for s in seqs) + 3
    literals = bytes((65 + k + i) & 255 for i in range(n))
    specs = [{PRE: None, RLE: {LL: 2, OF: 2, ML: 1}[w], FSE: FSE_SPEC[w], REP: None}[modes[w]] for w in (LL, OF, ML)]
    f.compressed(Z.lit_raw(literals) if lit is None else lit(literals), literals, seqs, modes=modes, specs=specs, last=last)


def _blocks():
    out = []
    f = Frame()
    f.raw(b"abc")
    f.raw(b"")
    f.raw(b"def", last=True)
    out.append(_acc("empty_raw_block_in_the_middle", "blocks: an empty raw block that is not last", f, matches=False))
    for kind in ("raw", "RLE"):
        for n in (1, 131072):
            f = Frame()
            f.raw(b"<")
            f.raw(_pattern(n)) if kind == "raw" else f.rle(0xC3, n)
            f.raw(b">", last=True)
            out.append(_acc("%s_block_%d" % (kind.lower(), n), "blocks: %s block of %d bytes" % (kind, n), f, matches=False))
    f = Frame()
    f.raw(b"x")
    f.compressed(Z.lit_raw(b"abcd"), b"abcd", [(4, BLOCK_MAX - 4, 2 + 3)], last=True)
    out.append(_acc("compressed_block_131072", "blocks: a compressed block of exactly 131072 bytes", f))
    f = _seeded()
    data = _h5(40)
    f.compressed(Z.lit_huf(H5, data, 0), data, [(10, 5, 7 + 3), (5, 4, 11 + 3), (0, 6, 20 + 3)], modes=(FSE, FSE, FSE),
                 specs=(_spread(36, (10, 5, 0, 2)), _spread(5, (1, 3, 4)), _spread(53, (0, 1, 2, 3, 6))), huf=H5)
    f.raw(b"raw between")
    f.rle(0x77, 33)
    data = _h5(30, 3)
    f.compressed(Z.lit_huf(H5, data, 0, treeless=True), data, [(5, 4, 2), (0, 9, 2), (2, 3, 3), (0, 4, 12 + 3)], modes=(REP, REP, REP), last=True)
    out.append(_acc("raw_and_rle_between_compressed", "blocks: raw and RLE blocks between compressed blocks keep the repeat offsets, the tree and the tables", f))
    f = _seeded()
    _mode_block(f, (FSE, FSE, FSE))
    f.compressed(Z.lit_raw(b"no sequences here"), b"no sequences here")
    f.compressed(Z.lit_raw(b"PQRST"), b"PQRST", [(2, 4, 2), (0, 4, 2), (2, 9, 3)], modes=(REP, REP, REP), last=True)
    out.append(_acc("no_sequences_between", "blocks: a block of 0 sequences between two with sequences is skipped by Repeat_Mode and the repeat offsets", f))
    return out


def _plain_literals():
    out = []
    for kind in ("raw", "RLE"):
        def lit(n, form, k=0):
            return (Z.lit_raw(_pattern(n, k), form), _pattern(n, k)) if kind == "raw" else (Z.lit_rle(0x41 + k, n, form), bytes([0x41 + k]) * n)
        for form, n in ((1, 17), (2, 300), (3, 5000)):
            f = _seeded()
            f.compressed(*lit(n, form), [(n - 2, 5, 9 + 3)], last=True)
            out.append(_acc("%s_literals_%d_byte_header" % (kind.lower(), form), "%s literals: header of %d bytes" % (kind, form), f))
        f = _seeded()
        f.compressed(*lit(5, 2), [(5, 5, 9 + 3)])
        f.compressed(*lit(5, 3, 1), [(1, 5, 1)], last=True)
        out.append(_acc("%s_literals_non_minimal" % kind.lower(), "%s literals: size 5 in the 2-byte and the 3-byte form" % kind, f))
        f = _seeded()
        f.compressed(*lit(9, "1b"), [(9, 5, 9 + 3)], last=True)
        out.append(_acc("%s_literals_size_format_10" % kind.lower(), "%s literals: size format 10 of the 1-byte form" % kind, f))
        for n in (0, 31, 32, 4095, 4096):
            f = _seeded()
            f.compressed(*lit(n, None), [(n // 2, 7, 30 + 3)])
            f.compressed(*lit(n, None, 2), [], last=True)
            out.append(_acc("%s_literals_size_%d" % (kind.lower(), n), "%s literals: size %d" % (kind, n), f))
    return out


def _compressed_literals():
    out = []
    H2 = Huffman([1, 1])
    for form, n in ((0, 200), (1, 200), (2, 5000), (3, 20000)):
        f = _seeded()
        data = _h5(n, form)
        f.compressed(Z.lit_huf(H5, data, form), data, [(n // 3, 8, 40 + 3), (n // 3, 3, 1)], last=True)
        out.append(_acc("huf_size_format_%d" % form, "compressed literals: size format %d" % form, f))
    for n in (0, 1, 1023):                                            # (0 bytes: the reference decodes it, so this decoder has to)
        f = Frame()
        data = _h5(n, 1)
        f.compressed(Z.lit_huf(H5, data, 0), data, [], last=True)
        out.append(_acc("huf_one_stream_%d" % n, "compressed literals: one stream of %d bytes" % n, f, matches=False))
    for n in (6, 7, 8, 9, 1023):
        f = Frame()
        data = _h5(n, 2)
        f.compressed(Z.lit_huf(H5, data, 1), data, [(n - 1, 4, 2 + 3)], last=True)
        out.append(_acc("huf_four_streams_%d" % n, "compressed literals: four streams of %d bytes" % n, f))
    f = Frame()
    data = bytes((0, 1, 1, 0, 1, 0, 0, 1))
    section = Z.lit_huf(H2, data, 1)
    assert len(section) == 3 + 2 + 6 + 4                              # header, tree, jump table, four streams of one byte
    f.compressed(section, data, [])
    f.compressed(Z.lit_huf(H2, data[:3], 0, treeless=True), data[:3], [], last=True)
    out.append(_acc("huf_streams_of_one_byte", "compressed literals: streams of one byte", f, matches=False))
    f = Frame()
    for n in range(1, 9):                                             # n codes of one bit: the end mark is bit n % 8 of the last byte
        data = bytes((i * 3 + n) % 5 % 2 for i in range(n))
        assert len(H2.stream(data)) == n // 8 + 1 and H2.stream(data)[-1].bit_length() - 1 == n % 8
        f.compressed(Z.lit_huf(H2, data, 0), data, [], last=n == 8)
    out.append(_acc("huf_end_mark_positions", ["compressed literals: end mark in bit %d" % b for b in range(8)], f, matches=False))
    return out


def _one_tree(name, covers, weights, tree=None, n=300, symbols=None, form=0):
    h = Huffman(weights)
    symbols = symbols or [s for s, w in enumerate(weights) if w]
    data = bytes(symbols[(i * 7 + i // 5) % len(symbols)] for i in range(n))
    f = Frame()
    f.compressed(Z.lit_huf(h, data, form, tree=None if tree is None else tree(h)), data, [(n // 2, 6, 17 + 3)], last=True, huf=h)
    return _acc(name, covers, f)


def _trees():
    out = [_one_tree("tree_direct_2_symbols", ["tree: direct weights for 2 symbols", "tree: all codes of 1 bits"], [1, 1]),
           _one_tree("tree_direct_128_weights", "tree: 128 direct weights", [1] * 128 + [8]),
           _one_tree("tree_depth_11", "tree: depth 11", [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1], n=2000, form=2)]
    for bits in (2, 4, 7):
        out.append(_one_tree("tree_all_codes_%d_bits" % bits, "tree: all codes of %d bits" % bits, [1] * (1 << bits), n=700, form=1))
    # FSE-compressed weights.  13 weights 4 1 2 0 0 0 0 0 0 0 0 1 (3 implied): twelve coded, an even number; 0 x8, 1 x2, 2 x1, 4 x1
    w = [4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3]
    out.append(_one_tree("tree_fse_log_5_even", ["tree: FSE weights, accuracy log 5", "tree: FSE weights, an even number"], w, tree=lambda h: h.fse([20, 6, 3, 0, 3], 5)))
    out.append(_one_tree("tree_fse_log_6", "tree: FSE weights, accuracy log 6", w, tree=lambda h: h.fse([40, 12, 6, 0, 6], 6)))
    out.append(_one_tree("tree_fse_less_than_one", "tree: FSE weights, a less-than-one count", w, tree=lambda h: h.fse([26, 4, -1, 0, 1], 5)))
    w = [4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 1, 3]                         # eleven coded weights: an odd number
    out.append(_one_tree("tree_fse_odd", "tree: FSE weights, an odd number", w, tree=lambda h: h.fse([18, 8, 3, 0, 3], 5)))
    # weight 9 once, weight 1 128 times (the implied last weight is 8): the distribution is 0, 63, then seven zeros (flags 3, 3, 0), then a less-than-one count for weight 9
    out.append(_one_tree("tree_fse_zero_runs", "tree: FSE weights, zero-run flags 3 + 3 + k", [9] + [1] * 128 + [8], tree=lambda h: h.fse([0, 63, 0, 0, 0, 0, 0, 0, 0, -1], 6),
                         symbols=[0, 129, 5, 0, 128, 0, 77]))
    # 256 symbols of weight 1: 255 coded weights over a distribution that also names weight 0 (never used), so that one state of weight 1 reads a bit
    out.append(_one_tree("tree_all_256_symbols", "tree: all 256 symbols, the implied last weight is symbol 255", [1] * 256, tree=lambda h: h.fse([1, 31], 5), n=1500, form=2,
                         symbols=list(range(256))))
    return out


def _treeless():
    f = _seeded()
    d = [_h5(50, k) for k in range(6)]
    f.compressed(Z.lit_huf(H5, d[0], 0), d[0], [(20, 5, 33 + 3)], huf=H5)
    f.compressed(Z.lit_huf(H5, d[1], 0, treeless=True), d[1], [(30, 4, 1)])                       # directly behind the tree, one stream
    f.raw(b"a raw block")
    f.compressed(Z.lit_huf(H5, d[2], 1, treeless=True), d[2], [(0, 4, 1), (50, 3, 9 + 3)])      # behind a raw block, four streams
    f.compressed(Z.lit_raw(b"raw literals"), b"raw literals", [(3, 3, 2)])
    f.compressed(Z.lit_huf(H5, d[3], 2, treeless=True), d[3], [(7, 70, 3)])                       # behind a compressed block with raw literals
    f.compressed(Z.lit_huf(H5, d[4], 0, treeless=True), d[4], [], last=True)                      # two in a row
    return [_acc("treeless", ["treeless: " + s for s in ("directly behind the tree", "behind a raw block", "behind a compressed block with raw literals", "two in a row", "one stream",
                                                         "four streams")], f)]


def _sequence_counts():
    out = []
    for what, n, form in (("1", 1, None), ("127", 127, None), ("128", 128, None), ("0x7EFF", 0x7EFF, None), ("0x7F00", 0x7F00, None), ("0 in the 2-byte form", 0, 2),
                          ("5 in the 2-byte form", 5, 2)):
        f = Frame()
        f.raw(b"wxyz")
        # RLE tables: ll 0, ml 3, offset value 4 + x (offsets 1..4)
        seqs = [(0, 3, 4 + (3 if i % 5 else i % 4)) for i in range(n)]
        f.compressed(Z.lit_raw(b"!"), b"!", seqs, modes=(RLE, RLE, RLE), specs=(0, 2, 0), nseq_form=form, last=True)
        out.append(_acc("nseq_%s" % what.replace(" ", "_"), "sequence count: " + what, f, matches=n > 0))
    return out


def _table_modes():
    out = []
    f = _seeded()
    combos = [(a, b, c) for a in (PRE, RLE, FSE) for b in (PRE, RLE, FSE) for c in (PRE, RLE, FSE)]
    for k, modes in enumerate(combos):
        _mode_block(f, modes, last=k == 26, k=k)
    out.append(_acc("modes_27_combinations", "modes: every combination of predefined, RLE and FSE over the three tables", f))
    for m in (PRE, RLE, FSE):
        f = _seeded()
        _mode_block(f, (m, m, m))
        for w in (LL, OF, ML):
            modes = [m, m, m]
            modes[w] = REP
            _mode_block(f, tuple(modes), last=w == ML, k=w + 1)
        out.append(_acc("repeat_from_%s" % KIND[m], ["modes: %s repeated from a %s table" % (TABLE[w], KIND[m]) for w in (LL, OF, ML)], f))
    f = _seeded()
    _mode_block(f, (FSE, FSE, FSE))
    for k in range(3):
        _mode_block(f, (REP, REP, REP), last=k == 2, k=k + 1)
    out.append(_acc("repeat_chained", "modes: a repeat chained over three blocks", f))
    f = _seeded()
    _mode_block(f, (FSE, RLE, FSE))
    _mode_block(f, (PRE, PRE, PRE), k=1)
    f.raw(b"raw")
    f.compressed(Z.lit_rle(0x2E, 40), b"." * 40)
    _mode_block(f, (REP, REP, REP), k=2)                                                          # (repeats the predefined tables of two blocks back)
    f.raw(b"raw again")
    _mode_block(f, (FSE, RLE, FSE), k=3)
    f.compressed(Z.lit_raw(b""), b"")
    f.raw(b"")
    _mode_block(f, (REP, REP, REP), last=True, k=4)
    out.append(_acc("repeat_source_two_blocks_back", "modes: a source two blocks back behind a raw block and a block of 0 sequences", f))
    return out


def _fse_descriptions():
    out = []
    f = _seeded()
    _mode_block(f, (FSE, FSE, FSE), last=True)
    out.append(_acc("fse_log_5", "fse: accuracy log 5", f))
    f = Frame()
    f.rle(0x2B, 3000)
    f.raw(SEED)
    f.rle(0x2D, 3000)
    lit = _pattern(50)
    big = (dist(36, {0: 200, 2: 150, 5: 100, 9: -1, 20: 60, 35: -1}), 9), (dist(31, {1: 100, 2: 100, 3: 54, 12: -1, 30: -1}), 8), (dist(53, {0: 255, 1: 128, 6: 127, 40: -1, 52: -1}), 9)
    f.compressed(Z.lit_raw(lit), lit, [(2, 4, 5), (5, 9, 9), (0, 3, 2), (9, 67, 4096 + 40), (2, 4, 6), (24, 3, 3)], modes=(FSE, FSE, FSE), specs=big, last=True)
    out.append(_acc("fse_maximal_logs", ["fse: literal lengths at accuracy log 9", "fse: offsets at accuracy log 8", "fse: match lengths at accuracy log 9",
                                         "fse: less-than-one counts and zero runs", "fse: the highest symbols 35, 30 and 52"], f))
    f = _seeded()
    lit = _pattern(12)
    f.compressed(Z.lit_raw(lit), lit, [(2, 4, 4), (0, 7, 9), (0, 7, 5), (2, 4, 11), (2, 7, 6)], modes=(FSE, FSE, FSE),
                 specs=((dist(3, {0: 16, 2: 16}), 5), (dist(4, {2: 31, 3: 1}), 5), (dist(5, {1: 24, 4: 8}), 5)), last=True)
    out.append(_acc("fse_two_symbols", "fse: two symbols only", f))
    return out


def _symbol_values():
    lls = sorted({Z.LL_BASE[c] + x for c in range(36) for x in (0, (1 << Z.LL_BITS[c]) - 1)})
    mls = sorted({Z.ML_BASE[c] + x for c in range(53) for x in (0, (1 << Z.ML_BITS[c]) - 1)}, reverse=True)
    n = max(len(lls), len(mls))
    pairs = []
    for i in range(n):
        ll, ml = lls[i] if i < len(lls) else 0, mls[i] if i < len(mls) else 3
        if ll >= ml:
            ll = min(ll, BLOCK_MAX - ml)                              # (code 35 with all extra bits set does not fit a block: the largest that does)
        else:
            ml = min(ml, BLOCK_MAX - ll)
        pairs.append((ll, ml))
    assert {Z.ll_code(p[0])[0] for p in pairs} == set(range(36)) and {Z.ml_code(p[1])[0] for p in pairs} == set(range(53))
    f = _seeded(16)
    blocks, cur = [], []
    for p in pairs:
        if sum(a + b for a, b in cur) + sum(p) > BLOCK_MAX:
            blocks.append(cur)
            cur = []
        cur.append(p)
    blocks.append(cur)
    for k, blk in enumerate(blocks):
        nl = sum(a for a, _ in blk)
        seqs = [(a, b, 3 + 1 + (i * 5 + k) % 9) for i, (a, b) in enumerate(blk)]
        if nl <= 3000:
            lit, literals = Z.lit_raw(_pattern(nl, k)), _pattern(nl, k)
        else:
            lit, literals = Z.lit_rle(0x30 + k, nl), bytes([0x30 + k]) * nl
        f.compressed(lit, literals, seqs, last=k == len(blocks) - 1)
    return [_acc("values_ll_and_ml_codes", ["values: every literal-length code with its extra bits all 0 and all 1", "values: every match-length code with its extra bits all 0 and all 1"], f)]


def _history(f, blocks):
    for k in range(blocks):
        f.rle(0x61 + k, BLOCK_MAX)


def _offset_codes():
    f = _seeded(256)
    _history(f, 17)
    f.raw(SEED[:200])
    seqs = []
    for c in range(21):
        for x in sorted({0, (1 << c) - 1}):
            ofv = (1 << c) + x
            seqs.append((1, 5, ofv))
    lit = _pattern(sum(s[0] for s in seqs) + 2)
    f.compressed(Z.lit_raw(lit), lit, seqs, last=True)
    return [_acc("values_offset_codes_0_to_20", "values: offset codes 0 to 20 with their extra bits all 0 and all 1", f)]


def _repeat_offsets():
    out = []
    frames, items = [], []
    for v, ll in ((1, 2), (2, 2), (3, 2), (1, 0), (2, 0)):
        f = _seeded(16)
        f.compressed(Z.lit_raw(b"ABCDE"), b"ABCDE", [(ll, 5, v), (1, 4, 2), (0, 3, 1)], last=True)
        frames.append(f)
        items.append("repeat offsets, first sequence of a frame: value %d %s literals" % (v, "with" if ll else "without"))
    out.append(_acc("repeat_offsets_first_of_frame", items, frames))
    frames, items = [], []
    for v in (1, 2, 3):
        for ll in (2, 0):
            f = _seeded(16)
            f.compressed(Z.lit_raw(b"abc"), b"abc", [(1, 4, 9 + 3), (1, 4, 5 + 3), (1, 4, 7 + 3)])
            assert f.rep == [7, 5, 9]
            f.compressed(Z.lit_raw(b"ABCDE"), b"ABCDE", [(ll, 5, v), (1, 4, 2), (0, 3, 1), (1, 6, 3)], last=True)
            frames.append(f)
            items.append("repeat offsets, first sequence of a later block: value %d %s literals" % (v, "with" if ll else "without"))
    out.append(_acc("repeat_offsets_first_of_later_block", items, frames))
    f = _seeded(16)
    f.compressed(Z.lit_raw(b"abc"), b"abc", [(1, 4, 9 + 3), (1, 4, 5 + 3), (1, 4, 7 + 3)])
    f.compressed(Z.lit_raw(b""), b"", [(0, 3, 3), (0, 4, 3), (0, 5, 3)])                          # 7 - 1, - 1, - 1: all three offsets behind the block are symbolic
    assert f.rep == [4, 5, 6]
    f.raw(b"--")
    f.compressed(Z.lit_raw(b"XY"), b"XY", [(1, 6, 3), (0, 4, 3), (1, 5, 2)], last=True)
    out.append(_acc("repeat_offset_decremented_three_times", "repeat offsets: a symbolic offset decremented three times", f))
    return out


def _shapes():
    out = []
    f = _seeded()
    f.compressed(Z.lit_raw(b"abc"), b"abc", [(3, 10, 20 + 3)], last=True)
    out.append(_acc("shape_last_sequence_ends_the_block", "shapes: the last sequence ends the block", f))
    f = _seeded()
    f.compressed(Z.lit_raw(_pattern(90)), _pattern(90), [(0, 4, 20 + 3)], last=True)
    out.append(_acc("shape_literals_behind_the_last_sequence", "shapes: literals behind the last sequence", f))
    f = _seeded()
    f.compressed(Z.lit_raw(b""), b"", [(0, 3, 20 + 3), (0, 3, 1), (0, 3, 2)], last=True)
    out.append(_acc("shape_ll_0_ml_3", "shapes: ll 0 ml 3", f))
    f = Frame()
    f.raw(b"Q")
    f.compressed(Z.lit_raw(b""), b"", [(0, BLOCK_MAX, 1 + 3)], last=True)
    out.append(_acc("shape_one_match_of_131072", "shapes: one match of 131072 bytes at offset 1", f))
    return out


def _bitstreams():
    """RLE tables cost no state bits: a sequence is exactly the extra bits of its offset code, the stream n * k + 1 bits"""
    out = []
    for nbytes, k in ((1023, 16), (1024, 15), (1025, 16), (1032, 15), (2049, 16)):
        n = next(n for n in range(1, 3000) if (n * k + 1 + 7) // 8 == nbytes)
        f = Frame()
        f.rle(0x41, 70000)
        f.rle(0x42, BLOCK_MAX - 70000)
        seqs = [(0, 3, (1 << k) + (i * 40503 + nbytes * 977) % (1 << k)) for i in range(n)]
        size = f.compressed(Z.lit_raw(b"$"), b"$", seqs, modes=(RLE, RLE, RLE), specs=(0, k, 0), last=True)
        assert size == 2 + 2 + 1 + 3 + nbytes, (size, nbytes)                                    # literals, count, modes, three RLE symbols, the bitstream
        out.append(_acc("bitstream_%d_bytes" % nbytes, "bitstream: %d bytes" % nbytes, f))
    f = Frame()
    f.rle(0x41, 70000)
    f.rle(0x42, BLOCK_MAX - 70000)
    for k in range(8, 16):                                                                       # one sequence of k bits: the end mark is bit k % 8
        f.compressed(Z.lit_raw(b"$"), b"$", [(0, 3, (1 << k) + (0x5A5A5 & ((1 << k) - 1)))], modes=(RLE, RLE, RLE), specs=(0, k, 0), last=k == 15)
    out.append(_acc("bitstream_end_mark_positions", ["bitstream: end mark in bit %d" % b for b in range(8)], f))
    return out


GEOMETRY_STREAMS, GEOMETRY_BYTES = 4, 300_000


def _geometry():
    out = []
    for seed in range(GEOMETRY_STREAMS):
        rng = np.random.default_rng(1000 + seed)
        f = Frame()
        first = True
        while len(f.out) < GEOMETRY_BYTES:
            start, pos, rep, seqs, nl = len(f.out), len(f.out), list(f.rep), [], 0
            room = min(BLOCK_MAX, int(rng.integers(90_000, BLOCK_MAX + 1)))
            while True:
                ll = 0 if rng.random() < 0.4 else int(rng.integers(1, 13))
                ml = int(rng.integers(4, 701))
                if pos - start + ll + ml > room:
                    break
                at, r, ofv = pos + ll, rng.random(), None
                if r < 0.3:                                                                      # one of the three recent offsets
                    ofv = int(rng.integers(1, 4))
                elif r < 0.6:
                    ofv = 3 + int(rng.integers(1, 66))
                else:                                                                            # a source within 40 bytes of the block's start, on either side
                    ofv = 3 + at - (start + int(rng.integers(-40, 41)))
                off = Z.resolve(rep, ofv, ll)[0] if ofv >= 1 else 0
                if ofv < 1 or off < 1 or off > at:
                    ll, ofv = max(ll, 1), 3 + 1
                    at = pos + ll
                rep = Z.resolve(rep, ofv, ll)[1]
                seqs.append((ll, ml, ofv))
                nl += ll
                pos = at + ml
            nl += int(rng.integers(0, 30))
            literals = _h5(nl, seed) if seed % 2 == 0 else bytes(rng.integers(0, 256, size=nl, dtype=np.uint8))
            if seed % 2 == 0:
                lit = Z.lit_huf(H5, literals, 1 if nl < 1024 else 2, treeless=not first)
            else:
                lit = Z.lit_raw(literals)
            first = False
            f.compressed(lit, literals, seqs, huf=H5 if seed % 2 == 0 else None, last=len(f.out) + pos - start + (nl - sum(s[0] for s in seqs)) >= GEOMETRY_BYTES)
        out.append(_acc("geometry_%d" % seed, "geometry: seeded random sequences over three blocks", f, checksum=seed == 1))
    return out


# ---------------------------------------------------------------------------------------------- refused streams
def _seq_payload(lit, nseq, modes, descriptions, bitstream):
    """a compressed block's payload from its parts as bytes: for the parts the builder's tables cannot stand for"""
    return bytes(lit) + Z.nseq_bytes(nseq) + bytes([(modes[LL] << 6) | (modes[OF] << 4) | (modes[ML] << 2)]) + b"".join(bytes(d) for d in descriptions) + bytes(bitstream)


def _refused():
    out = []

    def add(name, item, stream, error=GC_ERR_CORRUPT, capacity=1 << 16, stricter=False):
        out.append(Case("refused_" + name, item, stream, capacity=capacity, error=error, stricter=stricter))

    def one(name, item, build, error=GC_ERR_CORRUPT, seed=16, capacity=1 << 16, **kw):
        """a frame without a content size: a seed block, then what `build` adds"""
        f = Frame()
        if seed:
            f.raw(SEED[:seed])
        build(f)
        add(name, item, fb(f, fcs=None, **kw), error, capacity)

    def block(payload):
        return lambda f: f.bare(2, payload, last=True)

    ok = Frame()
    ok.raw(b"a sound frame", last=True)
    # frame header
    add("reserved_header_bit", "frame header: the reserved bit", fb(ok, reserved=1))
    add("window_exponent_22", "frame header: a window exponent above 21", fb(ok, fcs=None, window=22 << 3), GC_ERR_PARAM)
    # block headers
    one("block_type_3", "block header: block type 3", lambda f: f.bare(3, b"abc", last=True))
    one("block_size_above_128k", "block header: a Block_Size above 128 KiB", block(Z.lit_raw(bytes(BLOCK_MAX - 2)) + b"\0"), capacity=1 << 18)
    one("input_ends_before_the_last_block", "block header: input that ends before the last block", lambda f: f.raw(b"not the last"))
    f = Frame()
    f.raw(b"first")
    f.raw(b"last, it says", last=True)
    f.raw(b"and more")
    add("last_block_flag_in_the_middle", "block header: a last-block flag on a middle block, with bytes following", fb(f, fcs=None))
    # content size and checksum
    add("content_shorter_than_its_size", "content size: content shorter than Frame_Content_Size", fb(ok, fcs=len(ok.out) + 5), capacity=4096)
    f = Frame()
    f.raw(bytes(100), last=True)
    add("content_longer_than_its_size", "content size: content longer than Frame_Content_Size", fb(f, single=True, fcs=50, fcs_bytes=1), capacity=4096)
    f = _seeded()
    f.compressed(Z.lit_raw(b"abc"), b"abc", [(1, 30, 60 + 3)])
    f.compressed(Z.lit_raw(b"abc"), b"abc", [(1, 30, 1)], last=True)
    add("content_longer_than_its_size_compressed", "content size: content longer than Frame_Content_Size", fb(f, fcs=len(f.out) - 20), capacity=4096)
    add("wrong_checksum", "checksum: a wrong checksum", fb(ok, checksum=True, checksum_value=(Z.xxh64(bytes(ok.out)) ^ 1) & 0xFFFFFFFF))
    # literals section
    data = _h5(40)
    whole = H5.stream(data)
    one("literals_header_longer_than_the_block", "literals: a header longer than the block", block(bytes([3 << 2, 0])))
    one("literals_above_128k", "literals: regenerated size above 128 KiB", block(Z.lit_rle(0x41, BLOCK_MAX + 1) + b"\0"), capacity=1 << 18)
    one("four_streams_of_5_bytes", "literals: four streams regenerating 5 bytes", block(Z.lit_huf(H5, data[:5], 1) + b"\0"))
    one("jump_table_past_the_payload", "literals: a jump table that runs past the payload", block(Z.lit_huf(H5, data, 1, payload=Z.four_streams(H5, data, jump=(500, 500, 500))) + b"\0"))
    three = Z.four_streams(H5, data)[:-len(H5.stream(data[30:]))]
    one("empty_fourth_stream", "literals: an empty fourth stream", block(Z.lit_huf(H5, data, 1, payload=three) + b"\0"))
    one("literal_stream_ends_in_0", "literals: a stream whose last byte is 0", block(Z.lit_huf(H5, data, 0, payload=whole[:-1] + b"\0") + b"\0"))
    one("literal_stream_with_bits_left", "literals: a stream with bits left over", block(Z.lit_huf(H5, data[:39], 0, payload=whole) + b"\0"))
    one("literal_stream_too_short", "literals: a stream that regenerates too few bytes", block(Z.lit_huf(H5, data, 0, payload=H5.stream(data[:39])) + b"\0"))
    one("treeless_without_a_tree", "literals: treeless literals with no earlier tree", block(Z.lit_huf(H5, data, 0, treeless=True) + b"\0"))
    # Huffman weights
    def tree(desc, symbol_bits=b"\x01"):
        return block(Z.lit_header_huf(2, 0, 1, len(desc) + len(symbol_bits)) + desc + symbol_bits + b"\0")
    one("weights_not_a_power_of_two", "weights: weights that do not complete a power of two", tree(Z.huf_direct([3, 1])))
    one("tree_depth_12", "weights: a depth of 12", tree(Z.huf_direct([12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1])))
    one("one_symbol_of_weight_1", "weights: fewer than two weight-1 symbols", tree(Z.huf_direct([2, 1])))
    one("fse_weights_log_7", "weights: FSE weights with accuracy log 7", tree(Z.huf_fse([4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1], [80, 24, 12, 0, 12], 7)))
    desc = Z.huf_fse([4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1], [20, 6, 3, 0, 3], 5, size_byte=2)[:3]
    one("weights_ncount_past_its_bytes", "weights: an NCount that overshoots", tree(desc))
    one("more_than_255_weights", "weights: more than 255 weights", tree(Z.huf_fse([1] * 258, [1, 31], 5)))
    # sequence headers
    lit = Z.lit_raw(b"abc")
    one("sequence_count_and_nothing_else", "sequences header: a sequence count with nothing behind it", block(lit + b"\1"))
    one("reserved_mode_bits", "sequences header: reserved mode bits", lambda f: f.compressed(lit, b"abc", [(1, 4, 2 + 3)], reserved=1, last=True) or setattr(f, "sound", False))
    one("no_sequences_and_another_byte", "sequences header: 0 sequences followed by another byte", lambda f: f.compressed(lit, b"abc", [], tail=b"\0", last=True))
    for w, sym in ((LL, 36), (ML, 53), (OF, 32)):
        d = [bytes([1]), bytes([2]), bytes([1])]
        d[w] = bytes([sym])
        one("rle_symbol_%d" % sym, "sequences header: an RLE symbol past the alphabet (%s)" % TABLE[w], block(_seq_payload(lit, 1, (RLE, RLE, RLE), d, b"\x05")))
    for w, log, n in ((LL, 10, 36), (OF, 9, 29), (ML, 10, 53)):
        d = [bytes([1]), bytes([2]), bytes([1])]
        d[w] = Z.ncount(dist(n, {0: (1 << log) - 1, 1: 1}), log)
        modes = [RLE, RLE, RLE]
        modes[w] = FSE
        one("accuracy_log_%d_%d" % (w, log), "sequences header: an accuracy log above the maximum (%s)" % TABLE[w], block(_seq_payload(lit, 1, modes, d, b"\xff\xff\xff\x01")))
    for w, n in ((LL, 37), (OF, 33), (ML, 54)):
        d = [bytes([1]), bytes([2]), bytes([1])]
        d[w] = Z.ncount(dist(n, {0: 16, 1: 15, n - 1: 1}), 5)
        modes = [RLE, RLE, RLE]
        modes[w] = FSE
        one("ncount_symbol_%d" % (n - 1), "sequences header: NCount symbols past the alphabet (%s)" % TABLE[w], block(_seq_payload(lit, 1, modes, d, b"\xff\xff\xff\x01")))
    one("repeat_mode_without_a_table", "sequences header: Repeat_Mode with no earlier table", lambda f: f.compressed(lit, b"abc", [(1, 4, 2 + 3)], modes=(REP, PRE, PRE), last=True))
    # sequence bitstream
    two = [Z.seq_codes(1, 4, 2 + 3), Z.seq_codes(1, 5, 1)]
    one("sequence_bitstream_ends_in_0", "sequence bitstream: a last byte of 0", lambda f: f.compressed(lit, b"abc", codes=two, tail=b"\0", last=True) or setattr(f, "sound", False))
    one("sequence_bitstream_not_used_up", "sequence bitstream: not used up", lambda f: f.compressed(lit, b"abc", codes=two, nseq=1, last=True) or setattr(f, "sound", False))
    one("sequence_bitstream_over_read", "sequence bitstream: over-read", lambda f: f.compressed(lit, b"abc", codes=two, nseq=3, last=True) or setattr(f, "sound", False))
    one("literal_lengths_past_the_literals", "sequence bitstream: literal lengths that sum past the literals", lambda f: f.compressed(lit, b"abc", [(2, 4, 2 + 3), (2, 4, 1)], last=True))
    # offsets
    one("offset_inside_the_first_block", "offsets: past the content produced, inside the first block", lambda f: f.compressed(lit, b"abc", [(3, 4, 4 + 3)], last=True), seed=0)
    one("offset_in_front_of_the_frame", "offsets: past the content produced, reaching in front of the frame", lambda f: f.compressed(lit, b"abc", [(1, 4, 18 + 3)], last=True))
    f = _seeded(16)
    f.compressed(lit, b"abc", [(1, 4, 40 + 3)], last=True)
    big = Frame()
    big.raw(SEED[:100], last=True)
    add("offset_into_the_frame_before", "offsets: past the content produced, into the content of the frame before", fb(big) + fb(f, fcs=None))
    one("repeat_offset_0_concrete", "offsets: a repeat offset that comes to 0, concrete", lambda f: f.compressed(lit, b"abc", [(1, 4, 1 + 3), (0, 4, 3)], last=True))
    one("repeat_offset_0_symbolic", "offsets: a repeat offset that comes to 0, symbolic", lambda f: f.compressed(lit, b"abc", [(0, 4, 3)], last=True))
    # what the decoder does not support: the reference refuses these streams as well (it has no dictionary to go with the id, and nothing lies 2 GiB back)
    add("dictionary_id", "unsupported: a nonzero dictionary id", fb(ok, did=5, did_bytes=1), GC_ERR_PARAM)
    f = _seeded(16)
    f.bare(2, _seq_payload(lit, 1, (RLE, RLE, RLE), [bytes([1]), bytes([31]), bytes([1])], b"\xff\xff\xff\xff\x01"), last=True)
    add("offset_code_31", "unsupported: an offset code of 31", fb(f, fcs=None), GC_ERR_PARAM)
    # stricter than the reference: RFC 8878 3.1.1.2.3 / 3.1.1.2.4 limit Block_Size and Block_Content to 128 KiB; the reference's one-pass decoder only checks a compressed
    # block's Block_Size, this decoder holds a block's content in 128 KiB of LDS and checks all three
    f = _seeded(16)
    f.raw(bytes(BLOCK_MAX + 1), last=True)
    add("raw_block_above_128k", "a raw block above 128 KiB", fb(f, fcs=None), capacity=1 << 18, stricter=True)
    f = _seeded(16)
    f.compressed(lit, b"abc", [(0, BLOCK_MAX, 1 + 3), (0, 3, 1)], last=True)
    f.sound = False
    add("block_content_above_128k", "block content above 128 KiB", fb(f, fcs=None), capacity=1 << 18, stricter=True)
    return out


ITEMS_REFUSED = (
    ["frame header: the reserved bit", "frame header: a window exponent above 21", "block header: block type 3", "block header: a Block_Size above 128 KiB",
     "block header: input that ends before the last block", "block header: a last-block flag on a middle block, with bytes following",
     "content size: content shorter than Frame_Content_Size", "content size: content longer than Frame_Content_Size", "checksum: a wrong checksum"] +
    ["literals: " + s for s in ("a header longer than the block", "regenerated size above 128 KiB", "four streams regenerating 5 bytes",
                                "a jump table that runs past the payload", "an empty fourth stream", "a stream whose last byte is 0", "a stream with bits left over",
                                "a stream that regenerates too few bytes", "treeless literals with no earlier tree")] +
    ["weights: " + s for s in ("weights that do not complete a power of two", "a depth of 12", "fewer than two weight-1 symbols", "FSE weights with accuracy log 7",
                               "an NCount that overshoots", "more than 255 weights")] +
    ["sequences header: " + s for s in ("a sequence count with nothing behind it", "reserved mode bits", "0 sequences followed by another byte", "Repeat_Mode with no earlier table")] +
    ["sequences header: %s (%s)" % (s, TABLE[w]) for s in ("an RLE symbol past the alphabet", "an accuracy log above the maximum", "NCount symbols past the alphabet") for w in (LL, OF, ML)] +
    ["sequence bitstream: " + s for s in ("a last byte of 0", "not used up", "over-read", "literal lengths that sum past the literals")] +
    ["offsets: past the content produced, " + s for s in ("inside the first block", "reaching in front of the frame", "into the content of the frame before")] +
    ["offsets: a repeat offset that comes to 0, concrete", "offsets: a repeat offset that comes to 0, symbolic", "unsupported: a nonzero dictionary id", "unsupported: an offset code of 31"] +
    list(STRICTER_THAN_THE_REFERENCE))


def build_cases():
    cases = []
    for group in (_frames, _blocks, _plain_literals, _compressed_literals, _trees, _treeless, _sequence_counts, _table_modes, _fse_descriptions, _symbol_values, _offset_codes,
                  _repeat_offsets, _shapes, _bitstreams, _geometry, _refused):
        cases += group()
    assert len({c.name for c in cases}) == len(cases)
    return cases


# ---------------------------------------------------------------------------------------------- the fixture
class Pinned:
    """what tests/golden/zstd_handmade.npz holds of one case"""
    def __init__(self, name, covers, stream, flags, sha, content):
        self.name, self.covers, self.stream = name, covers.split("\n"), stream
        self.accepted, self.matches, self.stricter, self.error, self.capacity, self.size = bool(flags[0]), bool(flags[1]), bool(flags[2]), int(flags[3]), int(flags[4]), int(flags[5])
        self.sha = sha.tobytes().hex() if self.accepted else None
        self.content = content

    @staticmethod
    def load(path):
        """the file holds a few arrays for all cases together (an array per case and field costs more in zip headers than the streams weigh)"""
        z = np.load(path)
        names, covers = z["names"].tobytes().decode().split("\0"), z["covers"].tobytes().decode().split("\0")
        flags, shas, streams, contents = z["flags"], z["shas"], z["streams"], z["contents"]
        s_at, c_at = np.concatenate([[0], np.cumsum(z["stream_sizes"])]), np.concatenate([[0], np.cumsum(np.maximum(z["content_sizes"], 0))])
        return [Pinned(names[i], covers[i], streams[s_at[i]:s_at[i + 1]], flags[i], shas[i], contents[c_at[i]:c_at[i + 1]].tobytes() if z["content_sizes"][i] >= 0 else None)
                for i in range(len(names))]

    def matches_content(self, got):
        got = bytes(got)
        return len(got) == self.size and (got == self.content if self.content is not None else hashlib.sha256(got).hexdigest() == self.sha)


@pytest.fixture(scope="module")
def pinned():
    return Pinned.load(FIXTURE)


@pytest.fixture(scope="module")
def built():
    return {c.name: c for c in build_cases()}


# ---------------------------------------------------------------------------------------------- CPU: the builder against the fixture and the reference
def test_fixture_names_every_item(pinned):
    """every item of the lists above is covered by a pinned case of the right kind, and no case names an item the lists do not hold"""
    covered_ok = {c for p in pinned if p.accepted for c in p.covers}
    covered_bad = {c for p in pinned if not p.accepted for c in p.covers}
    assert [i for i in ITEMS_ACCEPTED if i not in covered_ok] == []
    assert [i for i in ITEMS_REFUSED if i not in covered_bad] == []
    assert covered_ok <= set(ITEMS_ACCEPTED) and covered_bad <= set(ITEMS_REFUSED)
    assert sorted(c for p in pinned if p.stricter for c in p.covers) == sorted(STRICTER_THAN_THE_REFERENCE)
    assert all(p.error in (GC_ERR_CORRUPT, GC_ERR_PARAM, GC_ERR_DST_SMALL) for p in pinned if not p.accepted)
    assert os.path.getsize(FIXTURE) < 200 * 1024


def test_builder_regenerates_the_pinned_streams(pinned, built):
    for p in pinned:
        c = built[p.name]
        assert c.stream == p.stream.tobytes(), p.name
        assert (c.accepted, c.matches, c.stricter, c.error, c.capacity, c.covers) == (p.accepted, p.matches, p.stricter, p.error, p.capacity, p.covers), p.name
        if p.accepted:
            assert p.matches_content(c.content), "the model and the reference decoder disagree on " + p.name
    assert set(built) == {p.name for p in pinned}


def test_reference_decoder_agrees_with_the_fixture(O, pinned):
    if O.ref("zstd") is None:
        pytest.skip("oracle/_ref (reference zstd) is not built")
    for p in pinned:
        if p.accepted or p.stricter:
            got = O.ref_zstd_decompress(p.stream, p.capacity).tobytes()
            assert p.stricter or p.matches_content(got), p.name
        else:
            with pytest.raises(ValueError):
                O.ref_zstd_decompress(p.stream, p.capacity)


def test_model_details():
    """the builder's own arithmetic, where a slip would silently thin the cases out"""
    for ll in list(range(0, 300)) + [65535, 65536, 131071]:
        c, x = Z.ll_code(ll)
        assert Z.LL_BASE[c] + x == ll and x < (1 << Z.LL_BITS[c])
    for ml in list(range(3, 300)) + [65538, 65539, 131074]:
        c, x = Z.ml_code(ml)
        assert Z.ML_BASE[c] + x == ml and x < (1 << Z.ML_BITS[c])
    for w, (norm, log) in Z.DEFAULTS.items():
        t = Z.FseTable(norm, log)
        assert sorted(set(t.sym)) == list(range(len(norm)))
        for s in range(len(norm)):                                   # the states of a symbol tile the whole table: every next state has exactly one state in front
            assert sorted(v for u in t.states(s) for v in range(t.base[u], t.base[u] + (1 << t.nb[u]))) == list(range(1 << log))
    assert Z.xxh64(b"") == 0xEF46DB3751D8E999 and Z.xxh64(b"a") == 0xD24EC4F1A98C6E5B and Z.xxh64(bytes(range(101))) == Z.xxh64(bytearray(range(101)))
    assert Z.resolve([1, 4, 8], 3, 0) == (0, [0, 1, 4]) and Z.resolve([7, 5, 9], 1, 0) == (5, [5, 7, 9]) and Z.resolve([7, 5, 9], 3, 1) == (9, [9, 7, 5])
    assert Z.nseq_bytes(0x7EFF) == b"\xfe\xff" and Z.nseq_bytes(0x7F00) == b"\xff\x00\x00" and Z.nseq_bytes(5, 2) == b"\x80\x05"
    h = Z.Huffman([2, 1, 1])
    assert h.code == {1: (0, 2), 2: (1, 2), 0: (1, 1)} and h.stream(bytes([0, 1])) == bytes([0b1100])


# ---------------------------------------------------------------------------------------------- decoding
def _call(dec, stream, capacity, room):
    """-> (rc, bytes produced, the whole output buffer, which was filled with 0xA5)"""
    a = np.ascontiguousarray(np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream)
    out = np.full(room, 0xA5, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = dec._lib.gc_zstd_decompress_host(dec._ctx, a.ctypes.data, a.size, out.ctypes.data, capacity, C.byref(n))
    return rc, n.value, out


def _accepted(dec, cases, wide=None):
    for p in cases:
        if not p.accepted:
            continue
        rc, n, out = _call(dec, p.stream, p.capacity, p.capacity + 64)
        assert rc == 0, "%s: rc %d" % (p.name, rc)
        assert p.matches_content(out[:n].tobytes()), "%s: wrong content" % p.name
        assert (out[n:] == 0xA5).all(), p.name
        if wide is not None and p.matches:
            assert (dec.wide_rounds() > 0) == wide, p.name


def _good(cases):
    return next(p for p in cases if p.name == "treeless")


def _refused_cases(dec, cases):
    good = _good(cases)
    for p in cases:
        if p.accepted:
            continue
        rc, n, out = _call(dec, p.stream, p.capacity, p.capacity + 64)
        assert rc == p.error, "%s: rc %d, expected %d" % (p.name, rc, p.error)
        assert n == 0 and (out == 0xA5).all(), p.name
        rc, n, out = _call(dec, good.stream, good.capacity, good.capacity + 64)
        assert rc == 0 and good.matches_content(out[:n].tobytes()), "the context does not decode a good stream behind " + p.name


def _all_in_one(dec, cases, bad=None):
    """every accepted stream in one call, skippable frames between them (a frame that does not state its size closes a batch of launches; the others share theirs)"""
    acc = [p for p in cases if p.accepted]
    parts, frames = [], 0
    for i, p in enumerate(acc):
        if bad is not None and i == len(acc) // 2:
            parts.append(bad.stream.tobytes())
        parts.append(Z.skippable(i & 15, b"skip" * (i % 3)))
        parts.append(p.stream.tobytes())
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8)
    total = sum(p.size for p in acc)
    rc, got, out = _call(dec, blob, total, total + 64)
    if bad is not None:
        assert rc == bad.error and got == 0
        good = _good(cases)
        rc, n, out = _call(dec, good.stream, good.capacity, good.capacity + 64)
        assert rc == 0 and good.matches_content(out[:n].tobytes())
        return
    assert rc == 0 and got == total
    at = 0
    for p in acc:
        assert p.matches_content(out[at:at + p.size].tobytes()), p.name
        at += p.size
    assert (out[got:] == 0xA5).all()
    _, frames, _ = dec.scan(blob)
    assert frames > 64                                           # the index kernel's second workgroup


def _one_call_tests(dec_of, monkeypatch, cases):
    dec = dec_of()
    try:
        _all_in_one(dec, cases)
        _all_in_one(dec, cases, bad=next(p for p in cases if p.name == "refused_offset_inside_the_first_block"))
    finally:
        dec.close()
    monkeypatch.setenv("GC_ZD_BATCH_KIB", "64")
    dec = dec_of()
    try:
        _all_in_one(dec, cases)
    finally:
        dec.close()


COMBINATIONS = [(w, s) for w in ("0", "1") for s in ("0", "1")]


# ---- CPU: the emulator
@pytest.fixture(scope="module")
def emu_dec(pkg, emu_lib_path):
    d = pkg.ZstdDecoder(lib_path=emu_lib_path)
    yield d
    d.close()


def test_emu_accepted_streams(emu_dec, pinned):
    _accepted(emu_dec, pinned)


@pytest.mark.parametrize("wide,seqv", COMBINATIONS)
def test_emu_accepted_streams_every_path(pkg, emu_lib_path, pinned, monkeypatch, wide, seqv):
    monkeypatch.setenv("GC_ZD_WIDE", wide)
    monkeypatch.setenv("GC_ZD_SEQV", seqv)
    dec = pkg.ZstdDecoder(lib_path=emu_lib_path)
    try:
        _accepted(dec, pinned, wide=wide == "1")
    finally:
        dec.close()


def test_emu_all_in_one_call(pkg, emu_lib_path, pinned, monkeypatch):
    _one_call_tests(lambda: pkg.ZstdDecoder(lib_path=emu_lib_path), monkeypatch, pinned)


@pytest.mark.parametrize("wide", ["0", "1"])
def test_emu_refused_streams(pkg, emu_lib_path, pinned, monkeypatch, wide):
    monkeypatch.setenv("GC_ZD_WIDE", wide)
    dec = pkg.ZstdDecoder(lib_path=emu_lib_path)
    try:
        _refused_cases(dec, pinned)
    finally:
        dec.close()


# ---- GPU
@pytest.fixture(scope="module")
def gpu_dec(pkg, graft):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    graft.build_hip()
    d = pkg.ZstdDecoder(device=0)
    yield d
    d.close()


@pytest.mark.gpu
def test_gpu_accepted_streams(gpu_dec, pinned):
    _accepted(gpu_dec, pinned)


@pytest.mark.gpu
def test_gpu_refused_streams(gpu_dec, pinned):
    _refused_cases(gpu_dec, pinned)


@pytest.mark.gpu
def test_gpu_all_in_one_call(pkg, gpu_dec, pinned, monkeypatch):
    _one_call_tests(lambda: pkg.ZstdDecoder(device=0), monkeypatch, pinned)


@pytest.mark.gpu
@pytest.mark.parametrize("wide,seqv", COMBINATIONS)
def test_gpu_every_path(pkg, gpu_hooks_kw, pinned, monkeypatch, wide, seqv):
    monkeypatch.setenv("GC_ZD_WIDE", wide)
    monkeypatch.setenv("GC_ZD_SEQV", seqv)
    dec = pkg.ZstdDecoder(**gpu_hooks_kw)
    try:
        _accepted(dec, pinned, wide=wide == "1")
        _refused_cases(dec, pinned)
    finally:
        dec.close()
    _one_call_tests(lambda: pkg.ZstdDecoder(**gpu_hooks_kw), monkeypatch, pinned)
