"""A brotli reader that says what a stream holds, written from RFC 7932 (section numbers in the comments are the RFC's).  It is a test instrument: it decodes, and it
keeps everything an encoder decided on the way -- per stream WBITS, per meta-block its kind, MLEN, the header's length in bits, the block-type counts, NPOSTFIX, NDIRECT, the
context modes and maps, every prefix code as it was described (simple or complex, the code-length code, the code-length symbols with their repeats, the depths) and every
command (insert&copy symbol, lengths, distance symbol or "implied", the resolved distance, the bit offset, the literal tree of each literal).  It shares no code with the
encoder or the decoder of this project; the format's tables are those of tests/brotli_build.py.  The static dictionary (Appendix A) is handed in by the caller.

    inspect(data, dictionary=None)          one RFC 7932 stream -> Stream
    frames(data)                            a brotli-mt stream -> [(compressed size, hint, payload)]
"""
import struct

import numpy as np

import brotli_build as B


class Malformed(ValueError):
    pass


class Bits:
    """LSB-first bits (section 1.5.3)"""
    def __init__(self, data):
        self.data, self.n, self.pos = bytes(data) + b"\0" * 8, len(data) * 8, 0

    def peek(self, nb):
        i = self.pos >> 3
        return (int.from_bytes(self.data[i:i + 6], "little") >> (self.pos & 7)) & ((1 << nb) - 1)

    def get(self, nb):
        v = self.peek(nb)
        self.pos += nb
        if self.pos > self.n:
            raise Malformed("the stream ends inside a field")
        return v

    def align(self):
        pad = -self.pos & 7
        return self.get(pad) if pad else 0


class Code:
    """one prefix code as it was described (sections 3.4, 3.5)"""
    def __init__(self):
        self.kind, self.alpha, self.depths, self.nsym = None, 0, [], 0
        self.symbols, self.tree_select = None, None                   # simple: NSYM symbols in the order written
        self.skip, self.clc_lengths, self.clc_stored, self.cl_symbols = None, None, 0, None      # complex: HSKIP, the 18 lengths by symbol, how many were written, [(symbol, extra)]
        self.bits = 0                                                  # the description's length
        self.single = None

    def finish(self):
        """canonical code words (section 3.2) -> a table indexed by the next `top` bits of the stream"""
        used = [s for s, d in enumerate(self.depths) if d]
        self.nsym = len(used) if self.single is None else 1
        if self.single is not None:
            return self
        top = max(self.depths)
        kraft = sum(1 << (top - d) for d in self.depths if d)
        if kraft != 1 << top:
            raise Malformed("a prefix code whose Kraft sum is not 1")
        sym_t, len_t = np.zeros(1 << top, np.int32), np.zeros(1 << top, np.int32)
        code = 0
        for d in range(1, top + 1):
            for s in used:
                if self.depths[s] == d:
                    r = int(format(code, "0%db" % d)[::-1], 2)
                    sym_t[r::1 << d] = s
                    len_t[r::1 << d] = d
                    code += 1
            code <<= 1
        self.top, self.sym_t, self.len_t = top, sym_t.tolist(), len_t.tolist()
        return self

    def read(self, r):
        if self.single is not None:
            return self.single
        v = r.peek(self.top)
        r.pos += self.len_t[v]
        if r.pos > r.n:
            raise Malformed("the stream ends inside a symbol")
        return self.sym_t[v]

    def cost(self, counts):
        return sum(n * self.depths[s] for s, n in counts.items())


def read_code(r, alpha):
    c = Code()
    c.alpha, start = alpha, r.pos
    hskip = r.get(2)
    if hskip == 1:                                                      # section 3.4
        c.kind = "simple"
        nsym = r.get(2) + 1
        ab = B.alphabet_bits(alpha)
        c.symbols = [r.get(ab) for _ in range(nsym)]
        if any(s >= alpha for s in c.symbols) or len(set(c.symbols)) != nsym:
            raise Malformed("a simple code with a symbol outside the alphabet or a repeated one")
        c.depths = [0] * alpha
        if nsym == 1:
            c.single = c.symbols[0]
        else:
            if nsym == 4:
                c.tree_select = r.get(1)
            lens = {2: [1, 1], 3: [1, 2, 2], 4: [1, 2, 3, 3] if c.tree_select else [2, 2, 2, 2]}[nsym]
            for s, l in zip(c.symbols, lens):
                c.depths[s] = l
        c.bits = r.pos - start
        return c.finish()
    c.kind, c.skip = "complex", hskip                                   # section 3.5
    fixed = {}
    for l, (val, nb) in B.CLC_FIXED.items():
        fixed[(val, nb)] = l
    cl = [0] * 18
    space, nz = 32, 0
    for i in range(hskip, 18):
        for nb in (2, 3, 4):
            if (r.peek(nb), nb) in fixed:
                l = fixed[(r.peek(nb), nb)]
                r.get(nb)
                break
        else:
            raise Malformed("no code-length code length")
        cl[B.CLC_ORDER[i]] = l
        c.clc_stored = i + 1 - hskip
        if l:
            nz += 1
            space -= 32 >> l
            if space <= 0:
                break
    if nz != 1 and space != 0:
        raise Malformed("the code-length code is not complete")
    c.clc_lengths = cl
    clc = Code()
    clc.alpha, clc.depths = 18, list(cl)
    if nz == 1:
        clc.single = next(s for s, l in enumerate(cl) if l)
    clc.finish()
    c.clc = clc
    depths, syms = [], []
    prev, rep_sym, rep = 8, None, 0
    space = 32768
    while len(depths) < alpha and space > 0:
        s = clc.read(r)
        if s < 16:
            syms.append((s, 0))
            depths.append(s)
            rep_sym = None
            if s:
                prev = s
                space -= 32768 >> s
            continue
        extra = r.get(2 if s == 16 else 3)
        syms.append((s, extra))
        if rep_sym == s:
            old = rep
            rep = ((rep - 2) << (2 if s == 16 else 3)) + 3 + extra
            add = rep - old
        else:
            rep_sym, rep = s, 3 + extra
            add = rep
        if len(depths) + add > alpha:
            raise Malformed("a repeat beyond the alphabet")
        depths += [prev if s == 16 else 0] * add
        if s == 16:
            space -= add * (32768 >> prev)
    if space != 0:
        raise Malformed("code lengths that do not fill the code space")
    c.cl_symbols = syms
    c.depths = depths + [0] * (alpha - len(depths))
    c.bits = r.pos - start
    return c.finish()


def varlen8(r):
    if not r.get(1):
        return 0
    nb = r.get(3)
    return (1 << nb) + r.get(nb)


class ContextMap:
    def __init__(self):
        self.ntrees, self.map, self.rlemax, self.imtf, self.code, self.symbols = 1, None, 0, 0, None, None


def read_map(r, size):
    m = ContextMap()
    m.ntrees = varlen8(r) + 1
    m.map = [0] * size
    if m.ntrees == 1:
        return m
    m.rlemax = r.get(4) + 1 if r.get(1) else 0
    m.code = read_code(r, m.ntrees + m.rlemax)
    out, m.symbols = [], []
    while len(out) < size:
        s = m.code.read(r)
        if s == 0:
            m.symbols.append((0, 0))
            out.append(0)
        elif s <= m.rlemax:
            extra = r.get(s)
            m.symbols.append((s, extra))
            out += [0] * ((1 << s) + extra)
        else:
            m.symbols.append((s, 0))
            out.append(s - m.rlemax)
    if len(out) > size:
        raise Malformed("a zero run beyond the context map")
    m.imtf = r.get(1)
    if m.imtf:                                                          # section 7.3
        table = list(range(256))
        for i, v in enumerate(out):
            out[i] = table[v]
            table.insert(0, table.pop(v))
    m.map = out
    return m


class BlockCat:
    """one category of block types (section 6)"""
    def __init__(self):
        self.n, self.type, self.prev, self.left, self.type_code, self.count_code, self.first, self.switches = 1, 0, 1, 1 << 60, None, None, None, []

    def take(self, r):
        if self.left == 0:
            s = self.type_code.read(r)
            t = self.prev if s == 0 else (self.type + 1 if s == 1 else s - 2)
            if t >= self.n:
                t -= self.n
            self.prev, self.type = self.type, t
            cc = self.count_code.read(r)
            self.left = B.BLOCK_BASE[cc] + r.get(B.BLOCK_EXTRA[cc])
            self.switches.append((t, self.left))
        self.left -= 1
        return self.type


class Command:
    __slots__ = ("symbol", "insert", "copy", "dsym", "dextra", "distance", "bit", "trees", "dictionary", "ended", "cmd_type")

    def triple(self):
        """(insert length, copy length, distance); a command the meta-block's end cuts behind its literals has no copy"""
        return (self.insert, 0, 0) if self.ended else (self.insert, self.copy, self.distance)


class MetaBlock:
    def __init__(self):
        self.kind, self.last, self.mlen, self.nibbles, self.header_bits, self.bit, self.end_bit = None, 0, 0, 0, 0, 0, 0
        self.nbltypes, self.npostfix, self.ndirect, self.modes = (1, 1, 1), 0, 0, []
        self.ntreesl, self.ntreesd, self.lit_map, self.dist_map = 1, 1, None, None
        self.lit_codes, self.cmd_codes, self.dist_codes, self.cats = [], [], [], None
        self.commands, self.content, self.pad, self.skipped, self.start = [], b"", 0, b"", 0

    def triples(self):
        return [c.triple() for c in self.commands]


class Stream:
    def __init__(self):
        self.wbits, self.blocks, self.content, self.bits, self.size = 0, [], b"", 0, 0


def read_wbits(r):                                                      # section 9.1
    if not r.get(1):
        return 16
    n = r.get(3)
    if n:
        return 17 + n
    m = r.get(3)
    if m == 0:
        return 17
    if m == 1:
        raise Malformed("the reserved WBITS pattern")
    return 8 + m


def inspect(data, dictionary=None, header=True, wbits=None, prefix=b"", ring=(4, 11, 15, 16), open_end=False):
    """one stream (or, with header=False, a piece of one behind `prefix` bytes of content; open_end: the piece may end at a meta-block border without a last one) -> Stream"""
    r = Bits(data)
    st = Stream()
    st.wbits = read_wbits(r) if header else wbits
    out = bytearray(prefix)
    ring = list(ring)
    window = (1 << st.wbits) - 16
    while not (open_end and st.blocks and r.pos >= r.n):
        mb = MetaBlock()
        st.blocks.append(mb)
        mb.bit, mb.start = r.pos, len(out) - len(prefix)
        mb.last = r.get(1)
        if mb.last and r.get(1):
            mb.kind, mb.header_bits, mb.end_bit = "empty last", r.pos - mb.bit, r.pos
            break
        mb.nibbles = (4, 5, 6, 0)[r.get(2)]
        if mb.nibbles == 0:                                             # section 9.2: metadata
            mb.kind = "metadata"
            if r.get(1):
                raise Malformed("the reserved bit of a metadata meta-block")
            nb = r.get(2)
            n = 0
            if nb:
                n = r.get(8 * nb) + 1
                if nb > 1 and (n - 1) >> (8 * (nb - 1)) == 0:
                    raise Malformed("MSKIPLEN with a zero top byte")
            mb.pad = r.align()
            if mb.pad:
                raise Malformed("padding that is not zero")
            mb.header_bits = r.pos - mb.bit
            mb.skipped = r.data[r.pos >> 3:(r.pos >> 3) + n]
            r.pos += 8 * n
            if r.pos > r.n:
                raise Malformed("metadata beyond the stream")
            mb.end_bit = r.pos
            if mb.last:
                break
            continue
        mb.mlen = r.get(4 * mb.nibbles) + 1
        if mb.nibbles > 4 and (mb.mlen - 1) >> (4 * (mb.nibbles - 1)) == 0:
            raise Malformed("MLEN with a zero top nibble")
        if not mb.last and r.get(1):
            mb.kind = "stored"
            mb.pad = r.align()
            if mb.pad:
                raise Malformed("padding that is not zero")
            mb.header_bits = r.pos - mb.bit
            mb.content = r.data[r.pos >> 3:(r.pos >> 3) + mb.mlen]
            r.pos += 8 * mb.mlen
            if r.pos > r.n:
                raise Malformed("stored bytes beyond the stream")
            out += mb.content
            mb.end_bit = r.pos
            continue
        mb.kind = "compressed"
        cats = [BlockCat() for _ in range(3)]
        mb.cats = cats
        for c in cats:
            c.n = varlen8(r) + 1
            if c.n >= 2:
                c.type_code = read_code(r, c.n + 2)
                c.count_code = read_code(r, 26)
                cc = c.count_code.read(r)
                c.left = B.BLOCK_BASE[cc] + r.get(B.BLOCK_EXTRA[cc])
                c.first = c.left
        mb.nbltypes = tuple(c.n for c in cats)
        mb.npostfix = r.get(2)
        mb.ndirect = r.get(4) << mb.npostfix
        mb.modes = [r.get(2) for _ in range(cats[0].n)]
        mb.lit_map = read_map(r, 64 * cats[0].n)
        mb.dist_map = read_map(r, 4 * cats[2].n)
        mb.ntreesl, mb.ntreesd = mb.lit_map.ntrees, mb.dist_map.ntrees
        mb.lit_codes = [read_code(r, 256) for _ in range(mb.ntreesl)]
        mb.cmd_codes = [read_code(r, 704) for _ in range(cats[1].n)]
        dalpha = B.distance_alphabet(mb.npostfix, mb.ndirect)
        mb.dist_codes = [read_code(r, dalpha) for _ in range(mb.ntreesd)]
        mb.header_bits = r.pos - mb.bit
        end = len(out) + mb.mlen
        lmap, dmap, modes = mb.lit_map.map, mb.dist_map.map, mb.modes
        L0, L1 = B.LUT0, B.LUT1
        while len(out) < end:
            c = Command()
            c.bit, c.ended, c.dictionary, c.dsym, c.dextra, c.distance = r.pos, False, None, None, 0, None
            c.cmd_type = cats[1].take(r)
            c.symbol = mb.cmd_codes[c.cmd_type].read(r)
            ic, cc, implicit = B.command_fields(c.symbol)
            c.insert = B.INS_BASE[ic] + r.get(B.INS_EXTRA[ic])
            c.copy = B.COPY_BASE[cc] + r.get(B.COPY_EXTRA[cc])
            c.trees = []
            if len(out) + c.insert > end:
                raise Malformed("literals beyond MLEN")
            simple = cats[0].n == 1
            for _ in range(c.insert):
                t = 0 if simple else cats[0].take(r)
                p1 = out[-1] if len(out) > 0 else 0
                p2 = out[-2] if len(out) > 1 else 0
                mode = modes[t]
                ctx = (L0[p1] | L1[p2]) if mode == B.UTF8 else B.context_id(mode, p1, p2)
                tree = lmap[64 * t + ctx]
                c.trees.append(tree)
                out.append(mb.lit_codes[tree].read(r))
            mb.commands.append(c)
            if len(out) >= end:
                c.ended = True
                break
            if implicit:
                c.dsym = "implied"
                dcode = 0
            else:
                t = cats[2].take(r)
                dcode = mb.dist_codes[dmap[4 * t + min(c.copy, 5) - 2]].read(r)
                c.dsym = dcode
                c.dextra = r.get(B.distance_bits(dcode, mb.npostfix, mb.ndirect))
            d = B.distance_of(dcode, c.dextra, mb.npostfix, mb.ndirect, ring)
            if d <= 0:
                raise Malformed("a distance of %d" % d)
            c.distance = d
            max_dist = min(len(out), window)
            if d > max_dist:                                            # section 8
                if not 4 <= c.copy <= 24:
                    raise Malformed("a dictionary reference of length %d" % c.copy)
                if dictionary is None:
                    raise Malformed("the stream refers to the static dictionary and none was handed in")
                ident = d - max_dist - 1
                index, tr = ident & ((1 << B.NDBITS[c.copy]) - 1), ident >> B.NDBITS[c.copy]
                if tr >= 121:
                    raise Malformed("transform %d" % tr)
                word = B.transform(B.dictionary_word(dictionary, c.copy, index), tr)
                c.dictionary = (c.copy, index, tr)
                if len(out) + len(word) > end:
                    raise Malformed("a dictionary word beyond MLEN")
                out += word
                continue
            if dcode != 0:
                ring = [d] + ring[:3]
            if len(out) + c.copy > end:
                raise Malformed("a copy beyond MLEN")
            if d >= c.copy:
                out += out[len(out) - d:len(out) - d + c.copy]
            else:
                out += (bytes(out[-d:]) * (c.copy // d + 1))[:c.copy]
        mb.content = bytes(out[end - mb.mlen:end])
        mb.end_bit = r.pos
        if mb.last:
            break
    st.bits = r.pos
    st.size = (r.pos + 7) >> 3
    st.ring = ring
    st.content = bytes(out[len(prefix):])
    return st


def frames(data):
    """a brotli-mt stream -> [(compressed size, hint, payload)] (the 16-byte header: magic, 8, compressed size, "BR", 64 KiB units to allocate)"""
    data, out, at = bytes(data), [], 0
    while at < len(data):
        magic, eight, csize, br, hint = struct.unpack_from("<IIIHH", data, at)
        if magic != 0x184D2A50 or eight != 8 or br != 0x5242 or at + 16 + csize > len(data):
            raise Malformed("no brotli-mt frame header at %d" % at)
        out.append((csize, hint, data[at + 16:at + 16 + csize]))
        at += 16 + csize
    return out
