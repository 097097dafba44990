"""Hand-built brotli streams for the device decoder (`gc_brotli_dec.hip`): what RFC 7932 allows and the reference's encoder never writes.  tests/brotli_build.py writes the
streams from the RFC and models the content; tests/golden/brotli_handmade.npz pins every stream together with what the REFERENCE's decoder made of it (content, or its
refusal).  Every accepted stream must decode to the same bytes under the model, the reference decoder and this decoder; every refused stream -- one per check the kernel makes
by name -- must be refused by the reference and by this decoder with the kernel's own error class, leave the output buffer alone and leave the context usable.

CPU: the kernel under the SIMT emulator -- default settings, every kernel instance forced, the small-LDS path.  GPU: the product library (its own choice of instance, by the
number of chunks) and the hooks library (forced instances, small LDS).  `python tests/golden/make_brotli_handmade_fixture.py` regenerates the fixture.

The distance alphabet has 16 + (k << NPOSTFIX) + (48 << NPOSTFIX) symbols, k = 0..15: 64, 65 and 128 exist, 129 does not, so the size above a power of two is 130 here.
One stream stays out on purpose: codes of one symbol each whose commands produce nothing cost no input bits, so a decoder without a guard never returns."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brotli_build as B
from brotli_build import LSB6, MSB6, SIGNED, UTF8, Stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "brotli_handmade.npz")
GC_ERR_DST_SMALL, GC_ERR_CORRUPT = -4, -6
RING_D = 4096                                                    # the output ring of the smallest kernel instance

# ---------------------------------------------------------------------------------------------- what has to be covered (sections 2 and 3 of the issue), by name
ITEMS_ACCEPTED = (
    ["window: WBITS %d" % w for w in range(10, 25)] +
    ["window %d: %s" % (w, k) for w in (10, 11, 12) for k in ("a copy at exactly maxBack", "one byte further is dictionary word 0 with transform 0", "a ring code that yields maxBack")] +
    ["metadata of %d bytes at the start, between two compressed meta-blocks and before ISLASTEMPTY" % n for n in (0, 1, 256, 257, 65537)] +
    ["uncompressed meta-block of %s bytes, then context and near / far copies out of it" % n for n in ("1", "2", "ring + 100")] +
    ["MNIBBLES 5 with a 24-bit copy length", "MNIBBLES 6 with a 24-bit copy length", "insert length with 24 extra bits over a one-symbol literal code"] +
    ["prefix codes: %s" % s for s in ("simple codes of 1-4 symbols, both 4-symbol shapes", "HSKIP 2", "HSKIP 3", "a code-length code with one symbol", "chained 16s and 17s",
                                      "a 16 as the first symbol", "lengths 1..15 in one code", "all symbols of length 8 through a one-symbol code-length code",
                                      "distance alphabets of 64, 65, 128 and 130 symbols")] +
    ["context map: RLEMAX %d" % r for r in (0, 1, 6, 16)] + ["context map: IMTF on", "context map: IMTF off"] + ["context map: %d trees" % n for n in (2, 3, 64, 256)] +
    ["context map: a run that ends on the last entry", "context modes: four literal block types with the four modes, every SIGNED and UTF8 class boundary",
     "distance context map over 4 contexts x 3 block types with copy lengths 2, 3, 4, 5"] +
    ["block switching, %s: %s" % (c, k) for c in ("literals", "commands", "distances")
     for k in ("code 0 as the first switch", "code 1 wraps to type 0", "explicit codes", "2 types", "256 types", "count codes 0, 1, 17, 24, 25")] +
    ["literal switch that changes the mode directly behind a copy", "literal switch that changes the mode directly behind a dictionary word"] +
    ["distances: NPOSTFIX %d NDIRECT %d" % (np_, k << np_) for np_ in range(4) for k in (0, 1, 15)] +
    ["distances: all 16 ring codes", "distances: code 0 and dictionary references do not push", "distances: the implicit-distance command range", "distances: the ring carried over a meta-block border"] +
    ["dictionary: every transform on words of length %d" % n for n in range(4, 25)] +
    ["dictionary: transforms that leave nothing", "dictionary: uppercase transforms on 2- and 3-byte UTF-8 sequences", "dictionary: a word that ends exactly on the meta-block's end",
     "dictionary: a literal behind a word under each context mode"])
ITEMS_REFUSED = [
    "the reserved WBITS pattern", "a metadata reserved bit", "a top MSKIPBYTES byte of zero", "nonzero padding of metadata", "nonzero padding of an uncompressed meta-block",
    "a metadata length that runs past the input", "an uncompressed length that runs past the input", "a zero top MNIBBLES nibble", "a simple code with a symbol >= the alphabet size",
    "a simple code with a repeated symbol", "an over-subscribed code-length code", "an under-subscribed code-length code", "over-subscribed symbol lengths",
    "under-subscribed symbol lengths", "a repeat that runs past the alphabet", "a context-map run that runs past the map", "an insert that crosses the meta-block's end",
    "a copy that crosses the meta-block's end", "a dictionary word that crosses the meta-block's end", "a ring code that gives a distance <= 0",
    "a dictionary reference with copy length 3", "a dictionary reference with copy length 25", "a transform index of 121", "input that ends inside a symbol", "MLEN beyond the capacity"]


class Case:
    def __init__(self, name, covers, stream, content=None, capacity=None, error=None, needs_dictionary=False, small_lds=False):
        self.name, self.covers, self.stream, self.content = name, list(covers), bytes(stream), None if content is None else bytes(content)
        self.accepted = error is None
        self.error = error                                        # the error class of a refused stream
        self.capacity = capacity if capacity is not None else (max(len(content), 1) if content is not None else 1 << 16)
        self.needs_dictionary, self.small_lds = needs_dictionary, small_lds


def _done(name, covers, s, **kw):
    return Case(name, covers, s.bytes(), content=bytes(s.out), needs_dictionary=s.uses_dictionary, **kw)


TWO_TREES = dict(ntrees=2, map=[i % 2 for i in range(64)], rlemax=0, imtf=0)
SEED = bytes((i * 37 + 11) & 255 for i in range(300))


# ---------------------------------------------------------------------------------------------- accepted streams
def _windows(D):
    out = []
    for wb in range(10, 25):
        s = Stream(wb)
        s.compressed([dict(literals=b"window %02d!" % wb, copy=5, dist=3), dict(copy=4, implicit=True)], last=True)
        out.append(_done("wbits_%d" % wb, ["window: WBITS %d" % wb], s))
    for wb in (10, 11, 12):
        for kind, item in (("copy", "a copy at exactly maxBack"), ("dict", "one byte further is dictionary word 0 with transform 0"), ("ring", "a ring code that yields maxBack")):
            if kind == "dict" and D is None:
                continue
            s = Stream(wb, D)
            mb = s.max_back

            def run(s, kind=kind, mb=mb):
                s.command(bytes(range(65, 76)), mb + 5 - 11, dist=11)      # eleven letters repeated up to position maxBack + 5
                if kind == "copy":
                    s.command(b"", 5, dist=mb)
                    assert s.last_distance == mb and not s.uses_dictionary
                elif kind == "dict":
                    s.command(b"", 5, dist=mb + 1)
                    assert s.uses_dictionary and s.out[-5:] == B.dictionary_word(D, 5, 0)
                else:
                    s.command(b"", 4, dist=mb - 1)
                    s.command(b"", 5, dcode=5)                             # the last distance + 1
                    assert s.last_distance == mb
                s.command(b"!", 3, dist=2)
            s.compressed(run, last=True)
            out.append(_done("wbits_%d_%s_at_maxback" % (wb, kind), ["window %d: %s" % (wb, item)], s))
    return out


def _meta_block_kinds(D):
    out = []
    for n in (0, 1, 256, 257, 65537):
        s = Stream(18)
        pay = bytes((i * 7 + 3) & 255 for i in range(n))
        s.metadata(pay)
        s.compressed([dict(literals=b"metadata, A", copy=4, dist=7), dict(literals=b"b", copy=3, dist=2)], lit_map=TWO_TREES)
        s.metadata(pay)
        # the first literal's tree comes from the two bytes in front of the metadata; the ring codes name distances from there
        s.compressed([dict(literals=b"Zq", copy=3, dcode=1), dict(literals=b"x", copy=4, dcode=3), dict(copy=2, implicit=True)], lit_map=TWO_TREES)
        s.metadata(pay)
        s.last_empty()
        out.append(_done("metadata_%d" % n, ["metadata of %d bytes at the start, between two compressed meta-blocks and before ISLASTEMPTY" % n], s))
    for n, label in ((1, "1"), (2, "2"), (RING_D + 100, "ring + 100")):
        s = Stream(16)
        s.compressed([dict(literals=b"head of it", copy=3, dist=4)])
        s.uncompressed(bytes((i * 73 + 41) & 255 for i in range(n)))
        s.compressed([dict(literals=b"Q", copy=4, dist=1), dict(literals=b"r", copy=6, dist=n + 6), dict(literals=b"", copy=5, dist=n + 20), dict(literals=b"s", copy=3, dist=min(n, 3) + 12)],
                     last=True, lit_map=TWO_TREES)
        out.append(_done("uncompressed_%d" % n, ["uncompressed meta-block of %s bytes, then context and near / far copies out of it" % label], s))
    for nib in (5, 6):
        total = (1 << 20) if nib == 5 else (1 << 20) + 1
        s = Stream(22)
        s.compressed([dict(literals=b"nib%d!" % nib, copy=total - 5, dist=1)], last=True, nibbles=nib)
        out.append(_done("mnibbles_%d" % nib, ["MNIBBLES %d with a 24-bit copy length" % nib], s))
    s = Stream(22)
    s.compressed([dict(literals=b"\xA7" * ((1 << 20) + 1), copy=2, end=True)], last=True)
    out.append(_done("insert_24_extra_bits", ["insert length with 24 extra bits over a one-symbol literal code"], s))
    return out


# ---- prefix code shapes over the literal, the command and four distance alphabets
ALPHABETS = [("literal", 256, 0, 0), ("command", 704, 0, 0), ("distance 64", 64, 0, 0), ("distance 65", 65, 0, 1), ("distance 128", 128, 1, 16), ("distance 130", 130, 1, 18)]


def _spread(items, k):
    """k of the items, the first and the last among them"""
    items = list(items)
    if len(items) <= k:
        return items
    return [items[round(i * (len(items) - 1) / (k - 1))] for i in range(k)]


def _shape(shape, alpha, want):
    """-> (code maker, the symbols it gives a code word)"""
    if shape.startswith("simple"):
        n, sel = int(shape[6]), 1 if shape.endswith("b") else 0
        syms = _spread(want, 4)[:n] if n < 4 else _spread(want, 4)
        order = {1: [0], 2: [1, 0], 3: [2, 0, 1], 4: [3, 1, 0, 2] if not sel else [2, 0, 3, 1]}[n]
        syms = [syms[i] for i in order]
        return (lambda w, a: B.simple_code(w, a, syms, sel)), sorted(syms)
    if shape in ("hskip2", "hskip3"):
        k = 12 if shape == "hskip2" else 20                       # full codes of lengths {3, 4} / {4, 5}: the code length code has no use for the lengths it skips
        syms = _spread(want, k)
        lens = dict(zip(syms, B.complete_lengths(k)))
        return (lambda w, a: B.lengths_code(w, a, lens, hskip=int(shape[5]))), syms
    if shape == "one_clc":
        L = alpha.bit_length() - 1                                # 2^L symbols of length L fill the code; the list ends there
        return (lambda w, a: B.complex_code(w, a, {L: 3}, [L] * (1 << L))), list(range(1 << L))
    if shape == "chain":
        base = max(11, want[0])                                   # a long run of zeros, then one length 4 and fifteen repeats of it
        symbols = [(17, e) for e in B.chain(base, 3)] + [4] + [(16, e) for e in B.chain(15, 2)]
        assert len(B.chain(base, 3)) > 1 and len(B.chain(15, 2)) > 1
        return (lambda w, a: B.complex_code(w, a, B.clc_for(symbols), symbols)), list(range(base, base + 16))
    if shape == "first16":
        symbols = [(16, 1), 1, 2, 3, 4, 5, 6]                     # four times length 8, the length a 16 repeats when nothing is in front of it
        return (lambda w, a: B.complex_code(w, a, B.clc_for(symbols), symbols)), list(range(10))
    assert shape == "len1to15"
    syms = _spread(want, 16)
    lens = dict(zip(syms, list(range(1, 15)) + [15, 15]))
    return (lambda w, a: B.lengths_code(w, a, lens)), syms


def _exercise(s, kind, usable):
    """commands that decode symbols of the code under test"""
    if kind == "literal":
        use = bytes(_spread(usable, 30))
        for i in range(0, len(use), 5):
            s.command(use[i:i + 5], 2 + i % 3, dist=5 + i)
    elif kind == "command":
        letters = b"abcdefgh"
        for i, sym in enumerate(_spread(usable, 24)):
            ic, cc, implicit = B.command_fields(sym)
            ins = B.INS_BASE[ic] + ((1 << B.INS_EXTRA[ic]) - 1 if B.INS_EXTRA[ic] <= 4 else 1)
            cp = B.COPY_BASE[cc] + ((1 << B.COPY_EXTRA[cc]) - 1 if B.COPY_EXTRA[cc] <= 4 else 1)
            s.command((letters * (ins // 8 + 2))[i % 8:i % 8 + ins], cp, dist=9 + i, implicit=implicit)
            assert len(s.out) and B.command_symbol(B.length_code(B.INS_BASE, ins), B.length_code(B.COPY_BASE, cp), implicit) == sym
    else:
        n = 0
        for i, dcode in enumerate(usable):
            nb = B.distance_bits(dcode, s.npostfix, s.ndirect)
            for extra in ((1 << nb) - 1, 0):
                if 0 < s.peek_distance(dcode, extra) <= len(s.out):
                    s.command(bytes([65 + i % 26]), 3 + i % 4, dcode=dcode, dextra=extra)
                    n += 1
                    break
        assert n >= min(8, len(usable)), (n, len(usable))            # (a simple code: every symbol)


def _prefix_codes(D):
    out = []
    shapes = [("simple", ["simple1", "simple2", "simple3", "simple4a", "simple4b"], "simple codes of 1-4 symbols, both 4-symbol shapes"), ("hskip2", ["hskip2"], "HSKIP 2"),
              ("hskip3", ["hskip3"], "HSKIP 3"), ("one_symbol_clc", ["one_clc"], "a code-length code with one symbol"), ("chained_16_17", ["chain"], "chained 16s and 17s"),
              ("first_symbol_16", ["first16"], "a 16 as the first symbol"), ("lengths_1_to_15", ["len1to15"], "lengths 1..15 in one code")]
    for name, group, item in shapes:
        s = Stream(18)
        s.uncompressed(SEED)
        for kind, alpha, np_, nd in ALPHABETS:
            assert B.distance_alphabet(np_, nd) == alpha or not kind.startswith("distance")
            if kind == "literal":
                want = list(range(33, 250, 9)) + [255]
            elif kind == "command":
                want = list(range(130, 704, 28)) + [703]          # (the last symbol: 22 595 literals and a copy of 2 119 bytes)
            else:
                want = list(range(0, 28))                         # ring codes and the distances that lie inside what has been produced
            for shape in group:
                make, usable = _shape(shape, alpha, want)
                key = {"literal": "lit_codes", "command": "cmd_codes"}.get(kind, "dist_codes")
                s.compressed(lambda s_, k=kind.split()[0], u=usable: _exercise(s_, k, u), npostfix=np_, ndirect=nd, **{key: [make]})
        s.last_empty()
        covers = ["prefix codes: " + item, "prefix codes: distance alphabets of 64, 65, 128 and 130 symbols"]
        if name == "one_symbol_clc":
            covers.append("prefix codes: all symbols of length 8 through a one-symbol code-length code")
        out.append(_done("prefix_" + name, covers, s))
    return out


# ---- context maps and modes
CLASS_BYTES = bytes([0, 1, 15, 16, 63, 64, 127, 128, 191, 192, 239, 240, 254, 255,                                       # every class boundary of SIGNED
                     9, 10, 13, 31, 32, 33, 34, 37, 39, 40, 41, 44, 46, 47, 48, 57, 58, 61, 64, 65, 69, 66, 90, 91, 96, 97, 101, 98, 122, 123, 126, 127, 128, 129, 191, 192, 193, 223, 224, 225, 255, 0, 10])  # and of UTF8


def _contexts(D):
    out = []
    n = len(CLASS_BYTES)
    code, extra = B.length_code(B.BLOCK_BASE, n), n - B.BLOCK_BASE[B.length_code(B.BLOCK_BASE, n)]
    for rlemax, imtf, ntrees in ((0, 0, 2), (1, 1, 3), (6, 0, 64), (16, 1, 256)):
        s = Stream(18)
        # five literal block types: LSB6, MSB6, UTF8, SIGNED, and one that is never switched to, whose 64 entries are the run of zeros that ends the map
        cmap = [(i * 7) % ntrees for i in range(256)] + [0] * 64
        commands = []
        for t in range(4):
            commands += [dict(literals=CLASS_BYTES[:20], copy=3, dist=5), dict(literals=CLASS_BYTES[20:40], copy=2, dist=11), dict(literals=CLASS_BYTES[40:], copy=4, dist=17)]
        s.compressed(commands, last=True, modes=(LSB6, MSB6, UTF8, SIGNED, UTF8), lit_map=dict(ntrees=ntrees, map=cmap, rlemax=rlemax, imtf=imtf),
                     blocks=(dict(n=5, first=(code, extra), switches=[(1, code, extra)] * 3), None, None))
        met = {m: {c for mm, c in s.contexts_met if mm == m} for m in range(4)}
        assert {c >> 3 for c in met[SIGNED]} == set(range(8)) and {c & 7 for c in met[SIGNED]} == set(range(8)), met[SIGNED]
        assert {c >> 2 for c in met[UTF8]} == set(range(16)) and {c & 3 for c in met[UTF8]} == set(range(4)), met[UTF8]
        out.append(_done("context_modes_rlemax%d_imtf%d_trees%d" % (rlemax, imtf, ntrees),
                         ["context map: RLEMAX %d" % rlemax, "context map: IMTF %s" % ("on" if imtf else "off"), "context map: %d trees" % ntrees,
                          "context map: a run that ends on the last entry", "context modes: four literal block types with the four modes, every SIGNED and UTF8 class boundary"], s, small_lds=True))
    s = Stream(16)
    s.uncompressed(SEED[:64])
    dmap = [1, 2, 3, 4, 2, 3, 4, 1, 3, 4, 0, 0]
    commands = [dict(literals=bytes([97 + i]), copy=2 + i % 4, dist=3 + 2 * i + 7 * (i % 4)) for i in range(12)]
    s.compressed(commands, last=True, dist_map=dict(ntrees=5, map=dmap, rlemax=2, imtf=1), blocks=(None, None, dict(n=3, first=(0, 3), switches=[(1, 0, 3)] * 2)))
    out.append(_done("distance_context_map", ["distance context map over 4 contexts x 3 block types with copy lengths 2, 3, 4, 5"], s, small_lds=True))
    return out


# ---- block switching
def _switch_plan(n):
    """first block of 2, then: code 0 (the type "before" the first: 1), code 1 (n = 2: wraps to 0), an explicit code, an explicit code and a long block, code 1 (n = 256: wraps to 0)"""
    far = 0 if n == 2 else n - 1
    mid = 1 if n == 2 else 100
    return dict(n=n, first=(0, 1), switches=[(0, 1, 1), (1, 17, 5), (2 + mid, 0, 0), (2 + far, 24, 0), (1, 25, 0)]), [2, 6, 310, 1, 8433, 5], [0, 1, 2 % n, mid, far, (far + 1) % n]


def _switching(D):
    out = []
    for k, cat in enumerate(("literals", "commands", "distances")):
        for n in (2, 256):
            plan, counts, types = _switch_plan(n)
            s = Stream(18)
            s.uncompressed(SEED[:40])
            total = sum(counts)
            if k == 0:
                lmap = dict(ntrees=n, map=[t for t in range(n) for _ in range(64)], rlemax=6, imtf=1)

                def run(s):
                    for i in range(0, total, 7):
                        s.command(bytes(97 + (i + j) % 8 for j in range(min(7, total - i))), 2, dist=3)
                s.compressed(run, last=True, blocks=(plan, None, None), lit_map=lmap)
            elif k == 1:
                def run(s):
                    for i in range(total):
                        s.command(b"", 2 + i % 5, dist=3 + i % 3)
                s.compressed(run, last=True, blocks=(None, plan, None))
            else:
                dmap = dict(ntrees=n, map=[t for t in range(n) for _ in range(4)], rlemax=2, imtf=0)

                def run(s):
                    for i in range(total):
                        s.command(b"", 2, dist=3 + i % 11)
                s.compressed(run, last=True, blocks=(None, None, plan), dist_map=dmap)
            assert s.trace[k] == types and not s.blk[k].switches, (cat, n, s.trace[k], types)
            covers = ["block switching, %s: %s" % (cat, x) for x in ("code 0 as the first switch", "explicit codes", "%d types" % n, "count codes 0, 1, 17, 24, 25")]
            covers.append("block switching, %s: code 1 wraps to type 0" % cat)
            out.append(_done("switch_%s_%d_types" % (cat, n), covers, s))
    for behind in ("copy", "dictionary word"):
        if behind != "copy" and D is None:
            continue
        s = Stream(16, D)
        cmap = [(i * 7) % 3 for i in range(128)]

        def run(s, behind=behind):
            s.command(b"Hello,", 4, dist=3)                       # the block of six literals ends here; the next literal switches the type, and the mode with it
            first = dict(dist=2) if behind == "copy" else dict(dist=s.dictionary_distance(4, 77, 0))
            s.command(b"", 4, **first)
            s.command(b"\xC3\xA9", 4, **(dict(dist=5) if behind == "copy" else dict(dist=s.dictionary_distance(4, 300, 1))))
            s.command(b"\xF0z", 3, dist=4)
        s.compressed(run, last=True, modes=(UTF8, SIGNED), lit_map=dict(ntrees=3, map=cmap, rlemax=0, imtf=0),
                     blocks=(dict(n=2, first=(1, 1), switches=[(0, 0, 1), (0, 0, 3)]), None, None))
        assert s.uses_dictionary == (behind != "copy")
        out.append(_done("mode_switch_behind_%s" % behind.replace(" ", "_"), ["literal switch that changes the mode directly behind a %s" % behind], s))
    return out


# ---- distances
def _far_seed(s):
    """17 000 bytes whose period is 257: distances of up to 2^14 mean something"""
    s.compressed([dict(literals=bytes(range(97, 110)), copy=243, dist=13), dict(literals=b"#", copy=17000, dist=257)])


def _distances(D):
    out = []
    for np_ in range(4):
        for k in (0, 1, 15):
            nd = k << np_
            s = Stream(22)
            _far_seed(s)
            used = []

            def run(s, np_=np_, nd=nd, used=used):
                del used[:]
                codes = ([16, 15 + nd] if nd else []) + [16 + nd + (h << np_) + l for h in (0, 1, 2, 3, 6, 11, 14, 17) for l in sorted({0, (1 << np_) - 1})]
                for i, dcode in enumerate(codes):
                    nb = B.distance_bits(dcode, np_, nd)
                    for extra in sorted({0, (1 << nb) - 1}):
                        if s.peek_distance(dcode, extra) <= len(s.out):
                            s.command(bytes([48 + i % 10]), 3 + i % 5, dcode=dcode, dextra=extra)
                            used.append((dcode, extra))
            s.compressed(run, last=True, npostfix=np_, ndirect=nd)
            assert len(used) >= (2 if nd else 0) + 2 * 6 * (2 if np_ else 1), (np_, nd, len(used))
            assert not nd or {(16, 0), (15 + nd, 0)} <= set(used)
            out.append(_done("distance_npostfix%d_ndirect%d" % (np_, nd), ["distances: NPOSTFIX %d NDIRECT %d" % (np_, nd)], s))
    # all 16 ring codes
    s = Stream(16)
    used = []

    def run(s):
        del used[:]
        s.command(bytes(range(64, 104)), 2, dist=23)
        for i, dcode in enumerate([4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 1, 2, 3, 0, 3, 9, 14, 2, 0, 1]):
            assert 0 < s.peek_distance(dcode) <= len(s.out)
            s.command(bytes([48 + i]), 2 + i % 4, dcode=dcode)
            used.append(dcode)
    s.compressed(run, last=True)
    assert set(used) == set(range(16))
    out.append(_done("ring_codes", ["distances: all 16 ring codes"], s))
    if D is not None:
        s = Stream(16, D)

        def run(s):
            s.command(b"ring and dictionary:", 3, dist=7)
            s.command(b"", 5, dist=s.dictionary_distance(5, 10, 0))
            s.command(b"", 3, dcode=0)                            # still 7
            s.command(b"a", 4, dist=12)
            s.command(b"", 6, dist=s.dictionary_distance(6, 2000, 3))
            s.command(b"", 8, dist=s.dictionary_distance(8, 5, 12))
            s.command(b"b", 3, dcode=1)                           # 7: the words in between pushed nothing
            s.command(b"", 4, dist=s.dictionary_distance(4, 1, 6))
            s.command(b"", 2, implicit=True)                      # 7
            s.command(b"c", 3, dcode=2)                           # 7 again: the ring is 7, 12, 7, 4
            s.command(b"", 3, dcode=4)                            # 6
            assert s.ring == [6, 7, 7, 12], s.ring
        s.compressed(run, last=True)
        out.append(_done("ring_with_dictionary_references", ["distances: code 0 and dictionary references do not push"], s))
    s = Stream(16)
    s.uncompressed(SEED[:80])

    def run(s):
        s.command(b"", 2, dist=9)
        for ic in range(8):
            for cc in (0, 7, 8, 15):
                sym = B.command_symbol(ic, cc, True)
                assert sym < 128
                extra = (1 << B.COPY_EXTRA[cc]) - 1
                s.command(bytes(65 + (ic + j) % 26 for j in range(B.INS_BASE[ic] + (1 if B.INS_EXTRA[ic] else 0))), B.COPY_BASE[cc] + extra, implicit=True)
            s.command(b"", 3, dist=5 + 2 * ic)
    s.compressed(run, last=True)
    out.append(_done("implicit_distance_commands", ["distances: the implicit-distance command range"], s))
    s = Stream(16)
    s.compressed([dict(literals=bytes(range(64, 114)), copy=3, dist=31), dict(literals=b"a", copy=2, dist=19), dict(literals=b"b", copy=4, dist=42), dict(literals=b"c", copy=3, dist=8)])
    s.compressed([dict(literals=b"d", copy=5, implicit=True), dict(literals=b"e", copy=2, dcode=3), dict(literals=b"f", copy=3, dcode=2), dict(literals=b"g", copy=3, dcode=11), dict(copy=4, dcode=6)],
                 last=True, npostfix=1, ndirect=4)
    out.append(_done("ring_across_meta_blocks", ["distances: the ring carried over a meta-block border"], s))
    return out


# ---- the static dictionary
def _utf8_words(D):
    """per word length a few words that begin with / contain a 2-byte and a 3-byte UTF-8 sequence: found by scanning the dictionary"""
    found = {}
    for L in range(4, 25):
        for idx in range(1 << B.NDBITS[L]):
            w = B.dictionary_word(D, L, idx)
            for key, hit in (("begin2", 0xC2 <= w[0] < 0xE0), ("begin3", w[0] >= 0xE0), ("inside2", w[0] < 0x80 and any(0xC2 <= b < 0xE0 for b in w[1:-1])),
                             ("inside3", w[0] < 0x80 and any(b >= 0xE0 for b in w[1:-2]))):
                if hit and len(found.setdefault(key, [])) < 3 and all(l != L for l, _ in found[key]):
                    found[key].append((L, idx))
    return found


def _dictionary(D):
    if D is None:
        return []
    out = []
    for L in range(4, 25):
        s = Stream(22, D)
        nwords = 1 << B.NDBITS[L]

        def run(s, L=L, nwords=nwords):
            s.command(b"<", 2, dist=1)
            for t in range(121):
                for idx in (0, nwords - 1, (L * 2654435761 >> 7) % nwords):
                    s.command(b"", L, dist=s.dictionary_distance(L, idx, t))
        s.compressed(run, last=True)
        out.append(_done("dictionary_transforms_length_%d" % L, ["dictionary: every transform on words of length %d" % L], s))
    s = Stream(22, D)

    def run(s):
        s.command(b"[", 2, dist=1)
        for t, n in ((34, 4), (39, 5), (40, 6), (55, 7), (54, 9), (42, 4), (63, 5), (56, 6), (48, 7), (59, 8), (64, 9)):        # omit the first / the last n
            for L in range(4, n + 1):
                before = len(s.out)
                s.command(b"", L, dist=s.dictionary_distance(L, 3 * L, t))
                assert len(s.out) == before
        s.command(b"]", 2, dist=1)
    s.compressed(run, last=True)
    out.append(_done("dictionary_transforms_that_leave_nothing", ["dictionary: transforms that leave nothing"], s))
    words = _utf8_words(D)
    assert all(words.get(k) for k in ("begin2", "begin3", "inside2", "inside3")), words
    s = Stream(22, D)

    def run(s):
        for key in ("begin2", "begin3", "inside2", "inside3"):
            for L, idx in words[key]:
                for t in (9, 44, 4, 68, 30, 85):                  # uppercase first / all, also with a prefix or a suffix
                    s.command(b"|", L, dist=s.dictionary_distance(L, idx, t))
    s.compressed(run, last=True)
    out.append(_done("dictionary_uppercase_utf8", ["dictionary: uppercase transforms on 2- and 3-byte UTF-8 sequences"], s))
    s = Stream(16, D)
    s.compressed(lambda s: (s.command(b"end:", 9, dist=s.dictionary_distance(9, 100, 5))))
    s.compressed(lambda s: (s.command(b"", 5, dist=s.dictionary_distance(5, 7, 0))), last=True)
    out.append(_done("dictionary_word_ends_the_meta_block", ["dictionary: a word that ends exactly on the meta-block's end"], s))
    s = Stream(16, D)
    cmap = [(i * 7) % 5 for i in range(256)]

    def run(s):
        for t in range(4):
            s.command(b"ab", 4 + t, dist=s.dictionary_distance(4 + t, 50 + t, 0))
            s.command(b"cd", 6, dist=s.dictionary_distance(6, 9 + t, 44))
            s.command(b"\xE2\x82", 7, dist=s.dictionary_distance(7, 1000 + t, 2))
            s.command(b"z", 2, dist=3)
    s.compressed(run, last=True, modes=(LSB6, MSB6, UTF8, SIGNED), lit_map=dict(ntrees=5, map=cmap, rlemax=3, imtf=1), blocks=(dict(n=4, first=(1, 2), switches=[(1, 1, 2)] * 3), None, None))
    out.append(_done("dictionary_literal_behind_word_modes", ["dictionary: a literal behind a word under each context mode"], s, small_lds=True))
    return out


# ---------------------------------------------------------------------------------------------- refused streams: everything but the one defect is well formed
def _tail(s):
    s.compressed([dict(literals=b"well formed", copy=4, dist=5)], last=True)
    return s


def _refused(D):
    out = []

    def add(name, item, s, error=GC_ERR_CORRUPT, capacity=1 << 16, stream=None):
        out.append(Case("refused_" + name, [item], s.bytes() if stream is None else stream, capacity=capacity, error=error, needs_dictionary=s.uses_dictionary))
    s = Stream(header=False); s.w.put(0b0010001, 7); add("wbits_reserved", "the reserved WBITS pattern", _tail(s))
    s = Stream(); s.metadata(b"abc", reserved=1); add("metadata_reserved_bit", "a metadata reserved bit", _tail(s))
    s = Stream(); s.metadata(b"abcde", size_bytes=2); add("metadata_top_size_byte_zero", "a top MSKIPBYTES byte of zero", _tail(s))
    s = Stream(); s.metadata(b"abc", pad=0xFF); assert s.last_pad; add("metadata_padding", "nonzero padding of metadata", _tail(s))
    s = Stream(); s.uncompressed(b"abcdef", pad=0xFF); assert s.last_pad; add("uncompressed_padding", "nonzero padding of an uncompressed meta-block", _tail(s))
    s = Stream(); _ = s.compressed([dict(literals=b"abc", copy=2, dist=1)]); s.metadata(b"abc", declared=100); add("metadata_past_input", "a metadata length that runs past the input", s)
    s = Stream(); _ = s.compressed([dict(literals=b"abc", copy=2, dist=1)]); s.uncompressed(b"abc", declared=50); add("uncompressed_past_input", "an uncompressed length that runs past the input", s)
    s = Stream(); s.compressed([dict(literals=b"sixteen bytes:", copy=2, dist=3)], last=True, nibbles=5); add("mnibbles_top_zero", "a zero top MNIBBLES nibble", s)
    s = Stream(); s.compressed([dict(literals=b"abc", copy=3, dist=2)], last=True, ndirect=1, dist_codes=[lambda w, a: B.simple_code(w, a, [17, 100])])
    add("simple_symbol_too_large", "a simple code with a symbol >= the alphabet size", s)
    s = Stream(); s.compressed([dict(literals=b"AAA", copy=3, dist=2)], last=True, lit_codes=[lambda w, a: B.simple_code(w, a, [65, 65])])
    add("simple_repeated_symbol", "a simple code with a repeated symbol", s)
    s = Stream(); s.compressed([dict(literals=b"\x00\x01", copy=3, dist=2)], last=True, lit_codes=[lambda w, a: B.complex_code(w, a, {1: 1, 2: 2, 3: 1}, [1, 3, 3])])
    add("clc_oversubscribed", "an over-subscribed code-length code", s)
    s = Stream(); s.compressed([dict(literals=b"\x01\x02", copy=3, dist=2)], last=True, lit_codes=[lambda w, a: B.complex_code(w, a, {0: 2, 1: 2}, [0, 1, 1])])
    add("clc_undersubscribed", "an under-subscribed code-length code", s)
    s = Stream(); s.compressed([dict(literals=b"AC", copy=3, dist=2)], last=True, lit_codes=[lambda w, a: B.complex_code(w, a, {0: 1, 1: 2, 2: 2}, [0] * 65 + [1, 2, 1])])
    add("lengths_oversubscribed", "over-subscribed symbol lengths", s)
    two = dict(n=2, first=(0, 3))
    s = Stream(); s.compressed([dict(literals=b"AB", copy=3, dist=2)], last=True, blocks=(dict(two, type_code=lambda w, a: B.complex_code(w, a, {0: 1, 2: 1}, [2, 2, 2, 0])), None, None))
    add("lengths_undersubscribed", "under-subscribed symbol lengths", s)
    s = Stream(); s.compressed([dict(literals=b"AB", copy=3, dist=2)], last=True, blocks=(dict(two, type_code=lambda w, a: B.complex_code(w, a, {1: 1, 16: 1}, [1, (16, 3)])), None, None))
    add("repeat_past_alphabet", "a repeat that runs past the alphabet", s)
    s = Stream(); s.compressed([dict(literals=b"AB", copy=3, dist=2)], last=True, dist_map=dict(ntrees=2, map=[0] * 4, rlemax=3, imtf=0, symbols=[(3, 0)]))
    add("map_run_past_map", "a context-map run that runs past the map", s)
    s = Stream(); s.compressed([dict(literals=b"eight is", copy=2, dist=3)], last=True, mlen=5); add("insert_crosses_end", "an insert that crosses the meta-block's end", s)
    s = Stream(); s.compressed([dict(literals=b"abc", copy=10, dist=2)], last=True, mlen=8); add("copy_crosses_end", "a copy that crosses the meta-block's end", s)
    s = Stream(); s.compressed([dict(literals=b"ab", copy=2, dist=1), dict(copy=2, dcode=4), dict(literals=b"cd", copy=2, dist=1)], last=True, mlen=10); assert 0 in s.distances
    add("ring_distance_zero", "a ring code that gives a distance <= 0", s)
    for n, dist in ((3, 50), (25, 200)):
        s = Stream(); s.compressed([dict(literals=b"abc", copy=n, dist=dist), dict(literals=b"d", copy=2, dist=1)], last=True, mlen=12)
        add("dictionary_copy_length_%d" % n, "a dictionary reference with copy length %d" % n, s)
    if D is not None:
        s = Stream(16, D); s.compressed(lambda s: s.command(b"a", 10, dist=s.dictionary_distance(10, 4, 0)), last=True, mlen=5)
        add("dictionary_word_crosses_end", "a dictionary word that crosses the meta-block's end", s)
        s = Stream(16, D); s.compressed(lambda s: (s.command(b"a", 4, dist=s.dictionary_distance(4, 9, 121)), s.command(b"bcd", 2, dist=1)), last=True, mlen=9)
        add("transform_121", "a transform index of 121", s)
    s = Stream(); s.compressed([dict(literals=bytes(range(60, 100)), copy=4, dist=9), dict(literals=bytes(range(100, 60, -1)), copy=4, dist=9)], last=True)
    whole = s.bytes()
    add("truncated_inside_a_symbol", "input that ends inside a symbol", s, stream=whole[:len(whole) - 24])
    s = Stream(18); s.compressed([dict(literals=b"too large", copy=70000 - 9, dist=4)], last=True)
    add("mlen_beyond_capacity", "MLEN beyond the capacity", s, error=GC_ERR_DST_SMALL, capacity=1 << 16)
    return out


def build_cases(D):
    """every case; D: the static dictionary of RFC 7932 Appendix A (numpy uint8 / bytes) or None, and then only the cases that do without it"""
    D = None if D is None else bytes(bytearray(D))
    cases = []
    for group in (_windows, _meta_block_kinds, _prefix_codes, _contexts, _switching, _distances, _dictionary, _refused):
        cases += group(D)
    assert len({c.name for c in cases}) == len(cases)
    return cases


# ---------------------------------------------------------------------------------------------- the fixture
class Pinned:
    """what tests/golden/brotli_handmade.npz holds of one case"""
    def __init__(self, z, i):
        self.name = bytes(z["name%d" % i]).decode()
        self.covers = bytes(z["covers%d" % i]).decode().split("\n")
        self.stream = z["stream%d" % i]
        flags = z["flags%d" % i]
        self.accepted, self.needs_dictionary, self.small_lds, self.error, self.capacity = bool(flags[0]), bool(flags[1]), bool(flags[2]), int(flags[3]), int(flags[4])
        self.size = int(flags[5])
        self.sha = bytes(z["sha%d" % i]).hex() if self.accepted else None
        self.content = z["content%d" % i].tobytes() if ("content%d" % i) in z.files else None

    def matches(self, got):
        got = bytes(got)
        return len(got) == self.size and (got == self.content if self.content is not None else hashlib.sha256(got).hexdigest() == self.sha)


@pytest.fixture(scope="module")
def pinned():
    z = np.load(FIXTURE)
    return [Pinned(z, i) for i in range(int(z["n"]))]


@pytest.fixture(scope="module")
def dictionary(O):
    return O.ref_brotli_dictionary() if O.ref("brotli") is not None else None


@pytest.fixture(scope="module")
def built(dictionary):
    return {c.name: c for c in build_cases(dictionary)}


def _runnable(pinned, dictionary):
    return [p for p in pinned if dictionary is not None or not p.needs_dictionary]


# ---------------------------------------------------------------------------------------------- CPU: the builder against the fixture and the reference
def test_fixture_names_every_item(pinned):
    """every item of the issue's lists is covered by a pinned case of the right kind"""
    covered_ok = {c for p in pinned if p.accepted for c in p.covers}
    covered_bad = {c for p in pinned if not p.accepted for c in p.covers}
    assert [i for i in ITEMS_ACCEPTED if i not in covered_ok] == []
    assert [i for i in ITEMS_REFUSED if i not in covered_bad] == []
    assert (covered_ok | covered_bad) <= set(ITEMS_ACCEPTED) | set(ITEMS_REFUSED)
    assert os.path.getsize(FIXTURE) < 200 * 1024


def test_builder_regenerates_the_pinned_streams(pinned, built, dictionary):
    for p in _runnable(pinned, dictionary):
        c = built[p.name]
        assert c.stream == p.stream.tobytes(), p.name
        assert (c.accepted, c.needs_dictionary, c.small_lds, c.capacity, c.covers) == (p.accepted, p.needs_dictionary, p.small_lds, p.capacity, p.covers), p.name
        if p.accepted:
            assert p.matches(c.content), "the model and the reference decoder disagree on " + p.name
    if dictionary is not None:
        assert set(built) == {p.name for p in pinned}


def test_reference_decoder_agrees_with_the_fixture(O, pinned):
    if O.ref("brotli") is None:
        pytest.skip("oracle/_ref (reference brotli) is not built")
    for p in pinned:
        if p.accepted:
            assert p.matches(O.ref_brotli_decompress(p.stream, p.capacity).tobytes()), p.name
            assert p.matches(O.ref_brotlimt_decompress(np.frombuffer(B.frame(p.stream.tobytes(), p.size), dtype=np.uint8), p.capacity + 65536).tobytes()), p.name
        else:
            with pytest.raises(ValueError):
                O.ref_brotli_decompress(p.stream, p.capacity)


def test_model_details():
    """the builder's own arithmetic, where a slip would silently thin the cases out"""
    for np_ in range(4):
        for nd in (0, 1 << np_, 15 << np_):
            for d in list(range(1, 600)) + [4095, 4096, 65535, 1 << 20, (1 << 24) - 17]:
                code, extra = B.distance_code_for(d, np_, nd)
                assert code < B.distance_alphabet(np_, nd) and B.distance_of(code, extra, np_, nd, [4, 11, 15, 16]) == d
    for n in list(range(3, 200)) + [704]:
        assert B.expand([(17, e) for e in B.chain(n, 3)], 1 << 20) == {} and len(B.expand([5] + [(16, e) for e in B.chain(n, 2)], 1 << 20)) == n + 1
    for k in range(2, 300):
        for lens in (B.complete_lengths(k), B.skewed_lengths(k)):
            assert len(lens) == k and max(lens) <= 15 and sum(1 << (15 - l) for l in lens) == 1 << 15
    assert [B.command_fields(B.command_symbol(i, c, imp)) for i, c, imp in ((0, 0, True), (7, 15, True), (0, 0, False), (23, 23, False), (8, 16, False))] == \
        [(0, 0, True), (7, 15, True), (0, 0, False), (23, 23, False), (8, 16, False)]
    assert B.transform(b"hello", 0) == b"hello" and B.transform(b"hello", 49) == b"helling " and B.transform(b"\xc3\xa9a", 44) == b"\xc3\x89A" and B.transform(b"abcd", 34) == b""


# ---------------------------------------------------------------------------------------------- decoding
def _decoder(pkg, dictionary, **kw):
    d = pkg.BrotliDecoder(**kw)
    if dictionary is not None:
        d.set_dictionary(dictionary)
    return d


@pytest.fixture(scope="module")
def emu_dec(pkg, dictionary, emu_lib_path):
    d = _decoder(pkg, dictionary, lib_path=emu_lib_path)
    yield d
    d.close()


@pytest.fixture(scope="module")
def gpu_dec(pkg, dictionary, graft):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    graft.build_hip()
    d = _decoder(pkg, dictionary, device=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def gpu_hooks_dec(pkg, dictionary, gpu_hooks_kw):
    d = _decoder(pkg, dictionary, **gpu_hooks_kw)
    yield d
    d.close()


def _call(dec, stream, capacity, room):
    """-> (rc, bytes produced, the whole output buffer, which was filled with 0xA5)"""
    a = np.ascontiguousarray(np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream)
    out = np.full(room, 0xA5, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = dec._lib.gc_brotli_decompress_host(dec._ctx, a.ctypes.data, a.size, out.ctypes.data, capacity, C.byref(n))
    return rc, n.value, out


def _accepted(dec, cases):
    for p in cases:
        if not p.accepted:
            continue
        for framed in (False, True):
            stream = np.frombuffer(B.frame(p.stream.tobytes(), p.size), dtype=np.uint8) if framed else p.stream
            cap = ((p.size + 65535) >> 16 << 16) if framed else p.capacity
            cap = max(cap, 1 << 16) if framed else cap
            rc, n, out = _call(dec, stream, cap, cap + 4096)
            assert rc == 0, "%s (%s): rc %d" % (p.name, "framed" if framed else "bare", rc)
            assert p.matches(out[:n].tobytes()), "%s (%s): wrong content" % (p.name, "framed" if framed else "bare")
            assert (out[n:] == 0xA5).all(), p.name


def _refused_cases(dec, cases, good):
    for p in cases:
        if p.accepted:
            continue
        rc, n, out = _call(dec, p.stream, p.capacity, p.capacity + 4096)
        assert rc == p.error, "%s: rc %d, expected %d" % (p.name, rc, p.error)
        assert n == 0 and (out == 0xA5).all(), p.name
        rc, n, out = _call(dec, good.stream, good.capacity, good.capacity + 64)
        assert rc == 0 and good.matches(out[:n].tobytes()), "the context does not decode a good stream behind " + p.name


def _good(cases):
    return next(p for p in cases if p.name == "ring_codes")


def _all_in_one(dec, cases, repeat_to=None):
    """every accepted stream framed, all frames in one call (repeated cyclically to `repeat_to` chunks): the content is the contents in a row"""
    acc = [p for p in cases if p.accepted and (p.size < (1 << 20) or repeat_to is None)]
    order = acc if repeat_to is None else [acc[i % len(acc)] for i in range(repeat_to)]
    blob = np.frombuffer(b"".join(B.frame(p.stream.tobytes(), p.size) for p in order), dtype=np.uint8)
    chunks, n, cap, used = dec.scan(blob)
    assert n == len(order) and used == blob.size
    rc, got, out = _call(dec, blob, cap, cap + 64)
    assert rc == 0 and got == sum(p.size for p in order)
    at = 0
    for p in order:
        assert p.matches(out[at:at + p.size].tobytes()), p.name
        at += p.size
    assert (out[got:] == 0xA5).all()
    return order, n


def _pack_arms(order):
    """the pack kernel copies 16 bytes at a time when source and destination are both 16-byte aligned: sources are slots of the hints (multiples of 64 KiB), destinations
    the running sum of the sizes -- both arms occur if some chunk starts at a multiple of 16 and some does not"""
    at, aligned, unaligned = 0, 0, 0
    for p in order:
        if p.size:
            aligned += at % 16 == 0
            unaligned += at % 16 != 0
        at += p.size
    return aligned, unaligned


# ---- CPU: the emulator
def test_emu_accepted_streams(emu_dec, pinned, dictionary):
    _accepted(emu_dec, _runnable(pinned, dictionary))


@pytest.mark.parametrize("instance", [1, 2, 3, 4])
def test_emu_accepted_streams_every_kernel_instance(emu_dec, pinned, dictionary, monkeypatch, instance):
    monkeypatch.setenv("GC_BRD_INSTANCE", str(instance))
    _accepted(emu_dec, _runnable(pinned, dictionary))


def test_emu_accepted_streams_small_lds(emu_dec, pinned, dictionary, monkeypatch):
    """GC_BRD_LDS=3072: no decoding tables, no context tables (the slow literal path), prefix codes in pages of HBM"""
    monkeypatch.setenv("GC_BRD_LDS", "3072")
    _accepted(emu_dec, [p for p in _runnable(pinned, dictionary) if p.small_lds])


def test_emu_refused_streams(emu_dec, pinned, dictionary):
    cases = _runnable(pinned, dictionary)
    _refused_cases(emu_dec, cases, _good(cases))


def test_emu_all_in_one_launch(emu_dec, pinned, dictionary):
    order, n = _all_in_one(emu_dec, _runnable(pinned, dictionary))
    aligned, unaligned = _pack_arms(order)
    assert aligned > 0 and unaligned > 0 and n <= 256


# ---- GPU
@pytest.mark.gpu
def test_gpu_accepted_streams(gpu_dec, pinned, dictionary):
    _accepted(gpu_dec, _runnable(pinned, dictionary))


@pytest.mark.gpu
def test_gpu_refused_streams(gpu_dec, pinned, dictionary):
    cases = _runnable(pinned, dictionary)
    _refused_cases(gpu_dec, cases, _good(cases))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks,low,high", [(None, 1, 256), (300, 257, 512), (600, 513, 1024), (1100, 1025, 1 << 20)])
def test_gpu_all_in_one_launch(gpu_dec, pinned, dictionary, chunks, low, high):
    """the product library picks the kernel instance by the number of chunks: a (up to 256), b (512), c (1024), d (more)"""
    order, n = _all_in_one(gpu_dec, _runnable(pinned, dictionary), chunks)
    assert low <= n <= high
    aligned, unaligned = _pack_arms(order)
    assert aligned > 0 and unaligned > 0


@pytest.mark.gpu
@pytest.mark.parametrize("instance", [1, 2, 3, 4])
def test_gpu_accepted_streams_every_kernel_instance(gpu_hooks_dec, pinned, dictionary, monkeypatch, instance):
    monkeypatch.setenv("GC_BRD_INSTANCE", str(instance))
    cases = _runnable(pinned, dictionary)
    _accepted(gpu_hooks_dec, cases)
    _refused_cases(gpu_hooks_dec, cases, _good(cases))


@pytest.mark.gpu
def test_gpu_accepted_streams_small_lds(gpu_hooks_dec, pinned, dictionary, monkeypatch):
    monkeypatch.setenv("GC_BRD_LDS", "3072")
    _accepted(gpu_hooks_dec, [p for p in _runnable(pinned, dictionary) if p.small_lds])
