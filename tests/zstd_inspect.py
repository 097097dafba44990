"""A zstd frame READER in plain Python, written from RFC 8878 (section numbers in the comments are the RFC's) on the primitives of tests/zstd_build.py: the code tables, the
FSE decoding table, the repeat-offset rule.  It is no decoder for speed or for hostile input (what a frame may not hold trips an assertion); it is there to SAY what a frame
holds, field by field, so that a test of an encoder can assert which of its branches wrote a block -- not only that some decoder gets the content back.

    inspect(data) -> [FrameInfo]                          every frame of the stream, skippable frames left out
    FrameInfo     .content  .blocks  .header (dict)       .checksum (the stored 4 bytes as an int, or None)
    BlockInfo     .type ("raw" / "rle" / "compressed")  .size (Block_Size)  .last  .content
      compressed: .lit      LitInfo: .type ("raw" / "rle" / "compressed" / "treeless"), .size_format, .header_bytes, .streams (1 / 4), .regen, .comp,
                            .tree (None, or TreeInfo: .kind "direct" / "fse", .weights as stored, .lengths[256] (0 = absent), .max_bits, .desc_bytes)
                  .literals the literal bytes
                  .nseq, .nseq_bytes (1, 2, 3: the form of the count)
                  .modes    [LL, OF, ML] of zstd_build.MODE_*;  .logs the table logs (0 for RLE);  .norms the normalised counts (None for RLE: .rle_syms has the symbol)
                  .seqs     [(ll, ml, offset_value)] as coded;  .codes [(ll code, of code, ml code)]
                  .resolved [(ll, ml, offset, form)] behind the repeat offsets (3.1.1.5); form: "new", "rep1", "rep2", "rep3", "rep1-1"
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_build as Z
from zstd_build import LL, ML, OF

MAX_LOG = {LL: 9, OF: 8, ML: 9}
MAX_SYM = {LL: 35, OF: 31, ML: 52}
FORMS = ("rep1", "rep2", "rep3", "rep1-1")


class FwdReader:
    """4.1.1: bits in the order they were written, least significant first"""
    def __init__(self, data, pos=0):
        self.data, self.bit = bytes(data), pos * 8

    def peek(self, n):
        b = self.bit >> 3
        return (int.from_bytes(self.data[b:b + 8], "little") >> (self.bit & 7)) & ((1 << n) - 1)

    def read(self, n):
        v = self.peek(n)
        self.bit += n
        return v

    def bytes_used(self):
        return (self.bit + 7) >> 3


class BackReader:
    """4.1 / 4.2.2: a stream read from its end, the first bit being the one below the highest set bit of the last byte.  Bits in front of the stream's start read as 0;
    `pos` goes negative then (the over-read that ends FSE-compressed weights)."""
    def __init__(self, data):
        self.data = bytes(data)
        assert self.data and self.data[-1], "a backward stream ends with a byte that holds the end mark"
        self.pos = 8 * (len(self.data) - 1) + self.data[-1].bit_length() - 1

    def peek(self, n):
        lo = self.pos - n
        if lo >= 0:
            b = lo >> 3
            return (int.from_bytes(self.data[b:b + 8], "little") >> (lo & 7)) & ((1 << n) - 1)
        if self.pos <= 0:
            return 0
        return (int.from_bytes(self.data[:8], "little") & ((1 << self.pos) - 1)) << (n - self.pos)

    def read(self, n):
        v = self.peek(n) if n else 0
        self.pos -= n
        return v


def read_ncount(data, pos, max_log, max_sym):
    """4.1.1: an FSE table description at data[pos:] -> (normalised counts with -1 for "less than one", accuracy log, bytes used)"""
    r = FwdReader(data[pos:pos + 512])
    log = r.read(4) + 5
    assert log <= max_log, "accuracy log %d above %d" % (log, max_log)
    remaining, norm = 1 << log, []
    while remaining > 0:
        assert len(norm) <= max_sym, "more symbols than the table may hold"
        top = remaining + 1                                       # the value read is in 0..remaining+1 ... ("probability + 1", and one more for "less than one")
        bits = top.bit_length()
        low_limit = (1 << bits) - 1 - top                         # values below it take one bit less
        v = r.peek(bits)
        if (v & ((1 << (bits - 1)) - 1)) < low_limit:
            v &= (1 << (bits - 1)) - 1
            r.bit += bits - 1
        else:
            r.bit += bits
            if v >= (1 << (bits - 1)):
                v -= low_limit
        count = v - 1
        norm.append(count)
        remaining -= abs(count)
        if count == 0:                                            # 2-bit repeat flags: that many more zeros; 3 = and another flag
            while True:
                k = r.read(2)
                norm += [0] * k
                if k != 3:
                    break
    assert remaining == 0 and len(norm) <= max_sym + 1
    return norm, log, r.bytes_used()


class TreeInfo:
    pass


def read_tree(data, pos):
    """4.2.1: a Huffman tree description -> TreeInfo"""
    t = TreeInfo()
    hb = data[pos]
    if hb >= 128:                                                 # 4.2.1.1: direct, 4 bits per weight
        n = hb - 127
        raw = data[pos + 1:pos + 1 + (n + 1) // 2]
        w = []
        for b in raw:
            w += [b >> 4, b & 15]
        t.kind, t.weights, t.desc_bytes = "direct", w[:n], 1 + (n + 1) // 2
    else:                                                         # 4.2.1.2: FSE-compressed, two interleaved states, ended by the over-read
        body = data[pos + 1:pos + 1 + hb]
        norm, log, used = read_ncount(body, 0, 6, 12)
        tab = Z.FseTable(norm, log)
        r = BackReader(body[used:])
        s = [r.read(log), r.read(log)]
        w, k = [], 0
        while True:
            w.append(tab.sym[s[k]])
            s[k] = tab.base[s[k]] + r.read(tab.nb[s[k]])
            if r.pos < 0:
                w.append(tab.sym[s[k ^ 1]])
                break
            k ^= 1
            assert len(w) <= 255, "more than 255 weights"
        t.kind, t.weights, t.desc_bytes, t.fse_norm, t.fse_log = "fse", w, 1 + hb, norm, log
    total = sum(1 << (x - 1) for x in t.weights if x)
    assert total, "no weight at all"
    t.max_bits = total.bit_length()                               # the smallest power of two above the sum
    rest = (1 << t.max_bits) - total
    assert rest & (rest - 1) == 0, "the weights leave no power of two for the last one"
    allw = t.weights + [rest.bit_length()]
    assert t.max_bits <= 11 and len(allw) <= 256
    t.lengths = [(t.max_bits + 1 - x) if x else 0 for x in allw] + [0] * (256 - len(allw))
    t.all_weights = allw
    # the decoding table: lowest weights take the lowest code space, symbols in order
    t.table_sym, t.table_len = [0] * (1 << t.max_bits), [0] * (1 << t.max_bits)
    at = 0
    for x in range(1, t.max_bits + 1):
        for sym, ws in enumerate(allw):
            if ws == x:
                span = 1 << (x - 1)
                t.table_sym[at:at + span] = [sym] * span
                t.table_len[at:at + span] = [t.max_bits + 1 - x] * span
                at += span
    assert at == 1 << t.max_bits
    return t


def huf_stream(tree, data, count):
    r = BackReader(data)
    out = bytearray(count)
    ts, tl, mb = tree.table_sym, tree.table_len, tree.max_bits
    for i in range(count):
        v = r.peek(mb)
        out[i] = ts[v]
        r.pos -= tl[v]
    assert r.pos == 0, "a Huffman stream of %d symbols ends %d bits from its start" % (count, r.pos)
    return bytes(out)


class LitInfo:
    pass


def read_literals(data, pos, prev_tree):
    """3.1.1.3.1 -> (LitInfo, the literal bytes, bytes used)"""
    li = LitInfo()
    b0 = data[pos]
    ltype, sf = b0 & 3, (b0 >> 2) & 3
    li.type, li.size_format, li.tree, li.streams = ("raw", "rle", "compressed", "treeless")[ltype], sf, None, 0
    if ltype < 2:
        if sf in (0, 2):
            li.header_bytes, li.regen = 1, b0 >> 3
        elif sf == 1:
            li.header_bytes, li.regen = 2, int.from_bytes(data[pos:pos + 2], "little") >> 4
        else:
            li.header_bytes, li.regen = 3, int.from_bytes(data[pos:pos + 3], "little") >> 4
        p = pos + li.header_bytes
        li.comp = li.regen if ltype == 0 else 1
        lit = bytes(data[p:p + li.regen]) if ltype == 0 else bytes(data[p:p + 1]) * li.regen
        assert len(lit) == li.regen
        return li, lit, li.header_bytes + li.comp
    bits = (10, 10, 14, 18)[sf]
    li.header_bytes = (3, 3, 4, 5)[sf]
    v = int.from_bytes(data[pos:pos + li.header_bytes], "little") >> 4
    li.regen, li.comp = v & ((1 << bits) - 1), v >> bits
    li.streams = 1 if sf == 0 else 4
    p = pos + li.header_bytes
    body = bytes(data[p:p + li.comp])
    assert len(body) == li.comp
    if ltype == 2:
        li.tree = read_tree(body, 0)
        body = body[li.tree.desc_bytes:]
        tree = li.tree
    else:
        assert prev_tree is not None, "treeless literals with no tree in front"
        tree = prev_tree
    li.used_tree = tree
    if li.streams == 1:
        lit = huf_stream(tree, body, li.regen)
    else:
        s1, s2, s3 = struct.unpack("<HHH", body[:6])
        seg = (li.regen + 3) // 4
        parts, at = [], 6
        for k, sz in enumerate((s1, s2, s3, len(body) - 6 - s1 - s2 - s3)):
            assert sz > 0
            parts.append(huf_stream(tree, body[at:at + sz], seg if k < 3 else li.regen - 3 * seg))
            at += sz
        lit = b"".join(parts)
    return li, lit, li.header_bytes + li.comp


class BlockInfo:
    pass


class FrameInfo:
    pass


def _form(ofv, ll):
    return "new" if ofv > 3 else FORMS[ofv - 1 + (ll == 0)]


def read_compressed_block(blk, payload, state):
    """3.1.1.3: state = the frame so far (content, rep, tables, tree)"""
    blk.lit, blk.literals, p = read_literals(payload, 0, state["tree"])
    if blk.lit.type in ("compressed", "treeless"):
        state["tree"] = blk.lit.used_tree
    # 3.1.1.3.2.1: Number_of_Sequences
    b0 = payload[p]
    if b0 < 128:
        blk.nseq, blk.nseq_bytes = b0, 1
    elif b0 < 255:
        blk.nseq, blk.nseq_bytes = ((b0 - 128) << 8) + payload[p + 1], 2
    else:
        blk.nseq, blk.nseq_bytes = payload[p + 1] + (payload[p + 2] << 8) + 0x7F00, 3
    p += blk.nseq_bytes
    blk.modes, blk.logs, blk.norms, blk.rle_syms, blk.seqs, blk.codes, blk.resolved = None, None, None, None, [], [], []
    blk.seq_section_bytes = len(payload) - (p - blk.nseq_bytes)
    out = state["content"]
    start = len(out)
    if blk.nseq == 0:
        assert p == len(payload), "bytes behind a sequence count of 0"
    else:
        mb = payload[p]
        p += 1
        assert mb & 3 == 0, "reserved bits of the modes byte"
        blk.modes = [(mb >> 6) & 3, (mb >> 4) & 3, (mb >> 2) & 3]
        tabs, blk.logs, blk.norms, blk.rle_syms = [], [], [], []
        for w in (LL, OF, ML):
            m = blk.modes[w]
            if m == Z.MODE_PREDEFINED:
                norm, log = Z.DEFAULTS[w]
                t = Z.FseTable(norm, log)
            elif m == Z.MODE_RLE:
                assert payload[p] <= MAX_SYM[w]
                t = Z.FseTable.of_rle(payload[p])
                p += 1
            elif m == Z.MODE_FSE:
                norm, log, used = read_ncount(payload, p, MAX_LOG[w], MAX_SYM[w])
                p += used
                t = Z.FseTable(norm, log)
            else:
                t = state["tables"][w]
                assert t is not None, "Repeat_Mode with nothing to repeat"
            tabs.append(t)
            blk.logs.append(t.log)
            blk.norms.append(None if t.rle else list(t.norm))
            blk.rle_syms.append(t.sym[0] if t.rle else None)
        state["tables"] = tabs
        r = BackReader(payload[p:])
        st = [0, 0, 0]
        for w in (LL, OF, ML):
            st[w] = r.read(tabs[w].log)
        lp = 0
        for i in range(blk.nseq):
            llc, ofc, mlc = tabs[LL].sym[st[LL]], tabs[OF].sym[st[OF]], tabs[ML].sym[st[ML]]
            assert ofc <= 31
            ofv = (1 << ofc) + r.read(ofc)
            ml = Z.ML_BASE[mlc] + r.read(Z.ML_BITS[mlc])
            ll = Z.LL_BASE[llc] + r.read(Z.LL_BITS[llc])
            if i + 1 < blk.nseq:
                for w in (LL, ML, OF):
                    st[w] = tabs[w].base[st[w]] + r.read(tabs[w].nb[st[w]])
            assert r.pos >= 0, "the sequences bitstream is read past its start"
            blk.seqs.append((ll, ml, ofv))
            blk.codes.append((llc, ofc, mlc))
            off, state["rep"] = Z.resolve(state["rep"], ofv, ll)
            blk.resolved.append((ll, ml, off, _form(ofv, ll)))
            assert lp + ll <= len(blk.literals), "sequence %d takes more literals than the block has" % i
            out += blk.literals[lp:lp + ll]
            lp += ll
            assert 0 < off <= len(out), "sequence %d: offset %d with %d bytes of content" % (i, off, len(out))
            if off >= ml:
                out += out[len(out) - off:len(out) - off + ml]
            else:
                piece = bytes(out[len(out) - off:])
                out += (piece * (ml // off + 1))[:ml]
        assert r.pos == 0, "the sequences bitstream ends %d bits from its start" % r.pos
        out += blk.literals[lp:]
        blk.content = bytes(out[start:])
        assert len(blk.content) <= Z.BLOCK_MAX
        return
    out += blk.literals
    blk.content = bytes(blk.literals)


def inspect(data):
    data = bytes(data)
    frames, p = [], 0
    while p < len(data):
        magic = struct.unpack_from("<I", data, p)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:                      # 3.1.2: skippable
            p += 8 + struct.unpack_from("<I", data, p + 4)[0]
            continue
        assert magic == Z.MAGIC, "no frame at %d" % p
        f = FrameInfo()
        f.offset = p
        fhd = data[p + 4]
        p += 5
        fcs_flag, single, has_sum, did_flag = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
        assert fhd & 8 == 0, "reserved bit of the frame header descriptor"
        f.header = dict(single_segment=bool(single), checksum=bool(has_sum), window=None, dict_id=0, content_size=None)
        if not single:
            f.header["window"] = data[p]
            p += 1
        nd = (0, 1, 2, 4)[did_flag]
        f.header["dict_id"] = int.from_bytes(data[p:p + nd], "little")
        p += nd
        nf = (1 if single else 0, 2, 4, 8)[fcs_flag]
        if nf:
            f.header["content_size"] = int.from_bytes(data[p:p + nf], "little") + (256 if nf == 2 else 0)
        p += nf
        f.header_bytes = p - f.offset
        state = dict(content=bytearray(), rep=[1, 4, 8], tables=[None, None, None], tree=None)
        f.blocks = []
        while True:
            h = int.from_bytes(data[p:p + 3], "little")
            p += 3
            blk = BlockInfo()
            blk.last, btype, blk.size = bool(h & 1), (h >> 1) & 3, h >> 3
            assert btype != 3, "reserved block type"
            blk.type = ("raw", "rle", "compressed")[btype]
            blk.offset = p
            if btype == 0:
                blk.content = data[p:p + blk.size]
                assert len(blk.content) == blk.size
                state["content"] += blk.content
                p += blk.size
            elif btype == 1:
                blk.content = data[p:p + 1] * blk.size
                state["content"] += blk.content
                p += 1
            else:
                payload = data[p:p + blk.size]
                assert len(payload) == blk.size
                read_compressed_block(blk, payload, state)
                p += blk.size
            f.blocks.append(blk)
            if blk.last:
                break
        f.checksum = None
        if has_sum:
            f.checksum = struct.unpack_from("<I", data, p)[0]
            p += 4
        f.content = bytes(state["content"])
        if f.header["content_size"] is not None:
            assert f.header["content_size"] == len(f.content), "the frame states %d bytes and holds %d" % (f.header["content_size"], len(f.content))
        f.size = p - f.offset
        frames.append(f)
    return frames


def content(data):
    return b"".join(f.content for f in inspect(data))
