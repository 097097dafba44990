"""A brotli stream builder that is also the model of what a decoder must produce, written from RFC 7932 (section numbers in the comments are the RFC's).  It writes exactly
what it is told to write, valid or not: the hand-built streams of tests/test_brotli_dec_handmade.py come from here, and so do the streams no decoder may accept.

    BitWriter                       LSB-first bits (section 1.5.3)
    simple_code / complex_code      prefix codes (sections 3.4, 3.5); `Code` holds the canonical code words
    Stream                          stream header, meta-block headers, metadata, uncompressed meta-blocks, compressed meta-blocks with their commands; its state is the model:
                                    the output bytes, the last four distances, the block state per category, the literal context under all four modes
    frame                           the 16-byte brotli-mt header in front of one stream

The static dictionary (Appendix A) is handed in by the caller; the 121 transforms (Appendix B) are typed in below as data."""
import struct

# ---------------------------------------------------------------------------------------------- format tables
INS_BASE = [0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090, 2114, 6210, 22594]        # section 5
INS_EXTRA = [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24]
COPY_BASE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582, 1094, 2118]
COPY_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24]
# the eleven 64-symbol cells of the insert-and-copy alphabet: (first insert code, first copy code); cells 0 and 1 carry the implicit distance code 0
CELLS = [(0, 0), (0, 8), (0, 0), (0, 8), (8, 0), (8, 8), (0, 16), (16, 0), (8, 16), (16, 8), (16, 16)]
BLOCK_BASE = [1, 5, 9, 13, 17, 25, 33, 41, 49, 65, 81, 97, 113, 145, 177, 209, 241, 305, 369, 497, 753, 1265, 2289, 4337, 8433, 16625]    # section 6
BLOCK_EXTRA = [2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13, 24]
CLC_ORDER = [1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15]                                                # section 3.5
CLC_FIXED = {0: (0b00, 2), 1: (0b0111, 4), 2: (0b011, 3), 3: (0b10, 2), 4: (0b01, 2), 5: (0b1111, 4)}                     # the bit strings of section 3.5 as LSB-first numbers
NDBITS = [0, 0, 0, 0, 10, 10, 11, 11, 10, 10, 10, 10, 10, 9, 9, 8, 7, 7, 8, 7, 7, 6, 6, 5, 5]                             # section 8
DICT_OFFSET = [0] * 26
for _l in range(4, 25):
    DICT_OFFSET[_l + 1] = DICT_OFFSET[_l] + (_l << NDBITS[_l])
assert DICT_OFFSET[25] == 122784
LSB6, MSB6, UTF8, SIGNED = 0, 1, 2, 3                                                                                     # section 7.1


def _runs(*pairs):
    out = []
    for value, count in pairs:
        out += [value] * count
    return out


# section 7.1: Lut0 / Lut1 of the UTF8 mode, Lut2 of the SIGNED mode
LUT0 = (_runs((0, 9), (4, 2), (0, 2), (4, 1), (0, 18)) +
        [8, 12, 16, 12, 12, 20, 12, 16, 24, 28, 12, 12, 32, 12, 36, 12] + [44] * 10 + [32, 32, 24, 40, 28, 12] +
        [12, 48, 52, 52, 52, 48, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 24, 12, 28, 12, 12] +
        [12, 56, 60, 60, 60, 56, 60, 60, 60, 56, 60, 60, 60, 60, 60, 56, 60, 60, 60, 60, 60, 56, 60, 60, 60, 60, 60, 24, 12, 28, 12, 0] +
        [0, 1] * 32 + [2, 3] * 32)
LUT1 = _runs((0, 33), (1, 15), (2, 10), (1, 7), (2, 26), (1, 6), (3, 26), (1, 4), (0, 1), (0, 96), (2, 32))
LUT2 = _runs((0, 1), (1, 15), (2, 48), (3, 64), (4, 64), (5, 48), (6, 15), (7, 1))
assert len(LUT0) == len(LUT1) == len(LUT2) == 256


def context_id(mode, p1, p2):
    if mode == LSB6:
        return p1 & 63
    if mode == MSB6:
        return p1 >> 2
    if mode == UTF8:
        return LUT0[p1] | LUT1[p2]
    return (LUT2[p1] << 3) | LUT2[p2]


# Appendix B: (prefix, elementary transform, suffix).  I identity, F uppercase first, A uppercase all, ("L", n) omit the last n, ("O", n) omit the first n
I, F, A = "I", "F", "A"
def _L(n): return ("L", n)
def _O(n): return ("O", n)
TRANSFORMS = [
    (b"", I, b""), (b"", I, b" "), (b" ", I, b" "), (b"", _O(1), b""), (b"", F, b" "), (b"", I, b" the "), (b" ", I, b""), (b"s ", I, b" "), (b"", I, b" of "), (b"", F, b""),
    (b"", I, b" and "), (b"", _O(2), b""), (b"", _L(1), b""), (b", ", I, b" "), (b"", I, b", "), (b" ", F, b" "), (b"", I, b" in "), (b"", I, b" to "), (b"e ", I, b" "), (b"", I, b"\""),
    (b"", I, b"."), (b"", I, b"\">"), (b"", I, b"\n"), (b"", _L(3), b""), (b"", I, b"]"), (b"", I, b" for "), (b"", _O(3), b""), (b"", _L(2), b""), (b"", I, b" a "), (b"", I, b" that "),
    (b" ", F, b""), (b"", I, b". "), (b".", I, b""), (b" ", I, b", "), (b"", _O(4), b""), (b"", I, b" with "), (b"", I, b"'"), (b"", I, b" from "), (b"", I, b" by "), (b"", _O(5), b""),
    (b"", _O(6), b""), (b" the ", I, b""), (b"", _L(4), b""), (b"", I, b". The "), (b"", A, b""), (b"", I, b" on "), (b"", I, b" as "), (b"", I, b" is "), (b"", _L(7), b""), (b"", _L(1), b"ing "),
    (b"", I, b"\n\t"), (b"", I, b":"), (b" ", I, b". "), (b"", I, b"ed "), (b"", _O(9), b""), (b"", _O(7), b""), (b"", _L(6), b""), (b"", I, b"("), (b"", F, b", "), (b"", _L(8), b""),
    (b"", I, b" at "), (b"", I, b"ly "), (b" the ", I, b" of "), (b"", _L(5), b""), (b"", _L(9), b""), (b" ", F, b", "), (b"", F, b"\""), (b".", I, b"("), (b"", A, b" "), (b"", F, b"\">"),
    (b"", I, b"=\""), (b" ", I, b"."), (b".com/", I, b""), (b" the ", I, b" of the "), (b"", F, b"'"), (b"", I, b". This "), (b"", I, b","), (b".", I, b" "), (b"", F, b"("), (b"", F, b"."),
    (b"", I, b" not "), (b" ", I, b"=\""), (b"", I, b"er "), (b" ", A, b" "), (b"", I, b"al "), (b" ", A, b""), (b"", I, b"='"), (b"", A, b"\""), (b"", F, b". "), (b" ", I, b"("),
    (b"", I, b"ful "), (b" ", F, b". "), (b"", I, b"ive "), (b"", I, b"less "), (b"", A, b"'"), (b"", I, b"est "), (b" ", F, b"."), (b"", A, b"\">"), (b" ", I, b"='"), (b"", F, b","),
    (b"", I, b"ize "), (b"", A, b"."), (b"\xc2\xa0", I, b""), (b" ", I, b","), (b"", F, b"=\""), (b"", A, b"=\""), (b"", I, b"ous "), (b"", A, b", "), (b"", F, b"='"), (b" ", F, b","),
    (b" ", A, b"=\""), (b" ", A, b", "), (b"", A, b","), (b"", A, b"("), (b"", A, b". "), (b" ", A, b"."), (b"", A, b"='"), (b" ", A, b". "), (b" ", F, b"=\""), (b" ", A, b"='"),
    (b" ", F, b"='"),
]
assert len(TRANSFORMS) == 121


def _upper(w, i):
    """section 8: one step of the UTF-8 aware uppercasing -> bytes consumed"""
    if w[i] < 192:
        if 97 <= w[i] <= 122:
            w[i] ^= 32
        return 1
    if w[i] < 224:
        if i + 1 < len(w):
            w[i + 1] ^= 32
        return 2
    if i + 2 < len(w):
        w[i + 2] ^= 5
    return 3


def transform(word, t):
    pre, kind, suf = TRANSFORMS[t]
    w = bytearray(word)
    if kind == F:
        if w:
            _upper(w, 0)
    elif kind == A:
        i = 0
        while i < len(w):
            i += _upper(w, i)
    elif kind != I and kind[0] == "L":
        w = w[:max(0, len(w) - kind[1])]
    elif kind != I:
        w = w[kind[1]:]
    return bytes(pre) + bytes(w) + bytes(suf)


def dictionary_word(dictionary, length, index):
    at = DICT_OFFSET[length] + index * length
    return bytes(bytearray(dictionary[at:at + length]))


# ---------------------------------------------------------------------------------------------- bits and prefix codes
class BitWriter:
    def __init__(self):
        self.acc = 0
        self.n = 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits), (value, bits)
        self.acc |= value << self.n
        self.n += bits

    def align(self, fill=0):
        pad = -self.n % 8
        self.put(fill & ((1 << pad) - 1), pad)
        return pad

    def raw(self, data):
        assert self.n % 8 == 0
        self.acc |= int.from_bytes(bytes(data), "little") << self.n
        self.n += 8 * len(data)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def alphabet_bits(alpha):
    n = 0
    while (1 << n) < alpha:
        n += 1
    return n


class Code:
    """a prefix code: the canonical code words of section 3.2 from the lengths; one symbol alone is coded in zero bits"""
    def __init__(self, alpha, lengths, single=None):
        self.alpha = alpha
        self.single = single
        self.lengths = dict(lengths)
        self.words = {}
        code = 0
        for L in range(1, 16):
            for sym in sorted(s for s, l in self.lengths.items() if l == L):
                self.words[sym] = (code, L)
                code += 1
            code <<= 1

    def symbols(self):
        return [self.single] if self.single is not None else sorted(self.words)

    def put(self, w, sym):
        if self.single is not None:
            assert sym == self.single, (sym, self.single)
            return
        code, L = self.words[sym]
        w.put(int(format(code, "0%db" % L)[::-1], 2), L)          # code words go out from their most significant bit (section 1.5.3)


class Recorder:
    """stands in for a code while a meta-block is planned: takes any symbol and remembers it"""
    def __init__(self):
        self.used = []

    def put(self, w, sym):
        if sym not in self.used:
            self.used.append(sym)


def simple_code(w, alpha, syms, tree_select=0):
    """section 3.4: 1..4 symbols, written as given (not sorted, not checked)"""
    w.put(1, 2)
    w.put(len(syms) - 1, 2)
    for s in syms:
        w.put(s, alphabet_bits(alpha))
    if len(syms) == 1:
        return Code(alpha, {}, single=syms[0])
    if len(syms) == 4:
        w.put(tree_select, 1)
    lens = {2: [1, 1], 3: [1, 2, 2], 4: [1, 2, 3, 3] if tree_select else [2, 2, 2, 2]}[len(syms)]
    return Code(alpha, dict(zip(syms, lens)))


def expand(symbols, alpha):
    """the code lengths that a list of code length symbols stands for (section 3.5): n is a length, (16, extra) repeats the last non-zero length (8 at the start),
    (17, extra) repeats zero; a 16 directly behind a 16 (a 17 behind a 17) extends the run"""
    out, prev, rep, rep_len = [], 8, 0, None
    for s in symbols:
        if not isinstance(s, tuple):
            out.append(s)
            rep = 0
            if s:
                prev = s
            continue
        kind, extra = s
        bits, new_len = (2, prev) if kind == 16 else (3, 0)
        if rep_len != new_len:
            rep, rep_len = 0, new_len
        old = rep
        if rep > 0:
            rep = (rep - 2) << bits
        rep += extra + 3
        out += [new_len] * (rep - old)
    return {i: l for i, l in enumerate(out[:alpha]) if l}


def complex_code(w, alpha, cl_lengths, symbols, hskip=0):
    """section 3.5: HSKIP, the lengths of the code length code (from entry `hskip` of the fixed order until the code is full), then `symbols` under that code"""
    cl = [cl_lengths.get(i, 0) for i in range(18)] if isinstance(cl_lengths, dict) else list(cl_lengths)
    assert hskip in (0, 2, 3) and all(cl[CLC_ORDER[i]] == 0 for i in range(hskip))
    w.put(hskip, 2)
    space = 32
    for i in range(hskip, 18):
        v = cl[CLC_ORDER[i]]
        w.put(*CLC_FIXED[v])
        if v:
            space -= 32 >> v
            if space <= 0:
                break
    used = [i for i in range(18) if cl[i]]
    clc = Code(18, {}, single=used[0]) if len(used) == 1 else Code(18, {i: cl[i] for i in used})
    for s in symbols:
        kind = s[0] if isinstance(s, tuple) else s
        clc.put(w, kind)
        if isinstance(s, tuple):
            w.put(s[1], 2 if kind == 16 else 3)
    return Code(alpha, expand(symbols, alpha))


def complete_lengths(k):
    """k >= 2 lengths of a full code, as even as they come"""
    d = alphabet_bits(k)
    short = (1 << d) - k
    return [d - 1] * short + [d] * (k - short)


def skewed_lengths(k):
    """k >= 2 lengths of a full code with as many different lengths as fit: 1, 2, 3, ... and an even tail"""
    s = max(0, min(k - 2, 6))
    return list(range(1, s + 1)) + [s + l for l in complete_lengths(k - s)]


def chain(n, bits):
    """the extra values of directly following repeat symbols that give a run of n >= 3 (bits: 2 for symbol 16, 3 for 17)"""
    if n <= (1 << bits) + 2:
        return [n - 3]
    e = (n - 3) % (1 << bits)
    return chain(((n - 3 - e) >> bits) + 2, bits) + [e]


def length_symbols(lengths, alpha, rle=True):
    """code length symbols for {symbol: length}: zero runs as 17s (chained where they are long), everything else plain; trailing zeros are not written"""
    out, i, last = [], 0, max(lengths)
    while i <= last:
        if lengths.get(i, 0) == 0:
            j = i
            while lengths.get(j, 0) == 0:
                j += 1
            if rle and j - i >= 3:
                out += [(17, e) for e in chain(j - i, 3)]
            else:
                out += [0] * (j - i)
            i = j
        else:
            out.append(lengths[i])
            i += 1
    return out


def clc_for(symbols, skip=()):
    """lengths of a full code length code over the symbols that occur"""
    used = sorted({s[0] if isinstance(s, tuple) else s for s in symbols})
    assert not set(used) & set(skip)
    if len(used) == 1:
        return {used[0]: 1}
    return dict(zip(used, complete_lengths(len(used))))


def lengths_code(w, alpha, lengths, hskip=0, rle=True):
    syms = length_symbols(lengths, alpha, rle)
    return complex_code(w, alpha, clc_for(syms), syms, hskip)


def auto_code(w, alpha, used, rotate=0):
    """a code over the symbols `used`: simple where four symbols do, else a full code with lengths 1, 2, 3, ... handed out from the `rotate`-th symbol on"""
    used = sorted(used)
    if len(used) <= 1:
        return simple_code(w, alpha, used or [0])
    if len(used) <= 4 and not rotate:
        return simple_code(w, alpha, used, 0)
    k = len(used)
    lens = skewed_lengths(k)
    return lengths_code(w, alpha, {used[(i + rotate) % k]: lens[i] for i in range(k)})


def varlen8(w, v):
    """section 9.2: 0..255"""
    if v == 0:
        w.put(0, 1)
        return
    w.put(1, 1)
    nb = v.bit_length() - 1
    w.put(nb, 3)
    w.put(v - (1 << nb), nb)


def frame(stream, size):
    """the brotli-mt frame around one stream: magic, 8, compressed size, "BR", the content's size in units of 64 KiB (rounded up)"""
    return struct.pack("<IIIHH", 0x184D2A50, 8, len(stream), 0x5242, max(1, (size + 65535) >> 16)) + bytes(stream)


# ---------------------------------------------------------------------------------------------- commands and distances
def command_symbol(ins_code, copy_code, implicit):
    for cell, (i0, c0) in enumerate(CELLS):
        if i0 <= ins_code < i0 + 8 and c0 <= copy_code < c0 + 8 and (cell < 2) == bool(implicit):
            return (cell << 6) | ((ins_code - i0) << 3) | (copy_code - c0)
    raise ValueError("no insert-and-copy symbol for insert code %d, copy code %d%s" % (ins_code, copy_code, ", implicit distance" if implicit else ""))


def command_fields(sym):
    i0, c0 = CELLS[sym >> 6]
    return i0 + ((sym >> 3) & 7), c0 + (sym & 7), sym < 128


def length_code(base, n):
    return max(i for i, b in enumerate(base) if b <= n)


def distance_alphabet(npostfix, ndirect):
    return 16 + ndirect + (48 << npostfix)


def distance_bits(dcode, npostfix, ndirect):
    return 0 if dcode < 16 + ndirect else 1 + (((dcode - ndirect - 16) >> npostfix) >> 1)


def distance_of(dcode, extra, npostfix, ndirect, ring):
    """section 4; ring = the last distances, most recent first"""
    if dcode < 16:
        base = ring[0] if 4 <= dcode < 10 else ring[1]
        return ring[dcode] if dcode < 4 else base + [-1, 1, -2, 2, -3, 3][(dcode - 4) % 6]
    if dcode < 16 + ndirect:
        return dcode - 15
    v = dcode - ndirect - 16
    hcode, lcode = v >> npostfix, v & ((1 << npostfix) - 1)
    nb = 1 + (hcode >> 1)
    return ((((2 + (hcode & 1)) << nb) - 4 + extra) << npostfix) + lcode + ndirect + 1


def distance_code_for(dist, npostfix, ndirect):
    """-> (symbol, extra) that spell `dist` without the ring"""
    if dist <= ndirect:
        return 15 + dist, 0
    x = dist - ndirect - 1
    lcode, y = x & ((1 << npostfix) - 1), (x >> npostfix) + 4
    nb = y.bit_length() - 2
    hcode = 2 * (nb - 1) + ((y >> nb) & 1)
    return 16 + ndirect + (hcode << npostfix) + lcode, y & ((1 << nb) - 1)


def mtf_encode(values):
    table, out = list(range(256)), []
    for v in values:
        i = table.index(v)
        out.append(i)
        table.insert(0, table.pop(i))
    return out


def map_symbols(indexes, rlemax):
    """section 7.3: the symbols of a context map: (0, -) a zero, (s <= rlemax, extra) 2^s + extra zeros, (v + rlemax, -) the value v"""
    out, i = [], 0
    while i < len(indexes):
        if indexes[i]:
            out.append((indexes[i] + rlemax, 0))
            i += 1
            continue
        j = i
        while j < len(indexes) and indexes[j] == 0:
            j += 1
        n = j - i
        while n:
            s = min(rlemax, n.bit_length() - 1)
            if s == 0:
                out.append((0, 0))
                n -= 1
            else:
                take = min(n, (2 << s) - 1)
                out.append((s, take - (1 << s)))
                n -= take
        i = j
    return out


class Blocks:
    """one category of block types (section 6)"""
    def __init__(self, spec):
        spec = spec or {}
        self.n = spec.get("n", 1)
        self.type_code = spec.get("type_code")            # callables (w, alpha) -> Code, or None: a code over the symbols the switches use
        self.count_code = spec.get("count_code")
        self.first = spec.get("first", (0, 0))            # (count code, extra) of the first block
        self.switches = list(spec.get("switches", ()))    # (type symbol, count code, extra), taken whenever a block runs out
        self.type, self.prev, self.left = 0, 1, 1 << 60


class Stream:
    """One brotli stream and the state of a decoder that has read it so far."""
    def __init__(self, wbits=16, dictionary=None, header=True):
        self.w = BitWriter()
        self.out = bytearray()
        self.ring = [4, 11, 15, 16]
        self.wbits = wbits
        self.dictionary = dictionary
        self.uses_dictionary = False
        self.contexts_met = set()                          # (mode, context id) of every literal
        self.distances = []                                # of every command that had one
        if header:
            self.put_wbits(wbits)

    # ---- section 9.1
    def put_wbits(self, wbits):
        if wbits == 16:
            self.w.put(0, 1)
        elif wbits == 17:
            self.w.put(0b0000001, 7)
        elif wbits >= 18:
            self.w.put(1 | ((wbits - 17) << 1), 4)
        else:
            self.w.put(1 | ((wbits - 8) << 4), 7)

    @property
    def max_back(self):
        return (1 << self.wbits) - 16

    @property
    def p1(self):
        return self.out[-1] if len(self.out) > 0 else 0

    @property
    def p2(self):
        return self.out[-2] if len(self.out) > 1 else 0

    # ---- section 9.2
    def meta_header(self, mlen, last, nibbles=None, uncompressed=0):
        w = self.w
        w.put(last, 1)
        if last:
            w.put(0, 1)
        nib = nibbles or (4 if mlen <= 1 << 16 else (5 if mlen <= 1 << 20 else 6))
        w.put(nib - 4, 2)
        for i in range(nib):
            w.put(((mlen - 1) >> (4 * i)) & 15, 4)
        if not last:
            w.put(uncompressed, 1)

    def last_empty(self):
        self.w.put(3, 2)

    def metadata(self, payload, size_bytes=None, declared=None, reserved=0, pad=0):
        """a meta-block that produces nothing: `payload` is skipped.  size_bytes: MSKIPBYTES; declared: the length written (the payload's own unless given)"""
        w, n = self.w, len(payload) if declared is None else declared
        w.put(0, 1)
        w.put(3, 2)
        w.put(reserved, 1)
        sb = size_bytes if size_bytes is not None else (0 if n == 0 else max(1, ((n - 1).bit_length() + 7) // 8))
        w.put(sb, 2)
        if sb:
            w.put(n - 1, 8 * sb)
        self.last_pad = w.align(pad)
        w.raw(payload)

    def uncompressed(self, data, declared=None, pad=0):
        self.meta_header(len(data) if declared is None else declared, 0, uncompressed=1)
        self.last_pad = self.w.align(pad)
        self.w.raw(data)
        self.out += data

    # ---- sections 9.2, 9.3: a compressed meta-block
    def compressed(self, commands, last=False, mlen=None, nibbles=None, blocks=(None, None, None), npostfix=0, ndirect=0, modes=(UTF8,), lit_map=None, dist_map=None,
                   lit_codes=None, cmd_codes=None, dist_codes=None, rotate=True):
        """commands: a list of dicts for command() -- or a function of the stream that issues them.  Codes that the caller does not give (callables (w, alpha) -> Code, per
        tree) are made over the symbols the commands use, found by a dry run; mlen likewise.  lit_map / dist_map: None (one tree) or dict(ntrees, map, rlemax, imtf,
        [code], [symbols]).  rotate: literal trees made here give the same byte another code word in every tree."""
        run = commands if callable(commands) else (lambda s: [s.command(**c) for c in commands])
        # the dry run: same state, recording codes
        saved = (bytearray(self.out), list(self.ring), self.w, self.uses_dictionary, set(self.contexts_met))
        self.w = BitWriter()
        self._begin(blocks, npostfix, ndirect, modes, lit_map, dist_map, 1 << 60)
        rec = {"L": [Recorder() for _ in range(self.ntrees[0])], "I": [Recorder() for _ in range(self.ntrees[1])], "D": [Recorder() for _ in range(self.ntrees[2])]}
        self.codes = rec
        for k in range(3):
            self.blk[k].type_code_obj = Recorder()
            self.blk[k].count_code_obj = Recorder()
        run(self)
        produced = len(self.out) - len(saved[0])
        planned = [(b.type_code_obj.used, b.count_code_obj.used) for b in self.blk]
        self.out, self.ring, self.w, self.uses_dictionary, self.contexts_met = saved
        # the real thing
        mlen = produced if mlen is None else mlen
        w = self.w
        self.meta_header(mlen, 1 if last else 0, nibbles)
        self._begin(blocks, npostfix, ndirect, modes, lit_map, dist_map, len(self.out) + mlen)
        for k, b in enumerate(self.blk):
            varlen8(w, b.n - 1)
            if b.n >= 2:
                b.type_code_obj = (b.type_code or (lambda w_, a, u=planned[k][0]: auto_code(w_, a, u)))(w, b.n + 2)
                b.count_code_obj = (b.count_code or (lambda w_, a, u=planned[k][1] + [b.first[0]]: auto_code(w_, a, set(u))))(w, 26)
                b.count_code_obj.put(w, b.first[0])
                w.put(b.first[1], BLOCK_EXTRA[b.first[0]])
        w.put(npostfix, 2)
        w.put(ndirect >> npostfix, 4)
        for m in self.modes:
            w.put(m, 2)
        self._put_map(lit_map)
        self._put_map(dist_map)
        lit_union = sorted({s for r in rec["L"] for s in r.used})
        self.codes = {"L": [], "I": [], "D": []}
        for kind, alpha, given in (("L", 256, lit_codes), ("I", 704, cmd_codes), ("D", distance_alphabet(npostfix, ndirect), dist_codes)):
            for t in range(len(rec[kind])):
                make = given[t] if given and t < len(given) and given[t] else None
                if make:
                    self.codes[kind].append(make(w, alpha))
                elif kind == "L" and rotate and len(rec["L"]) > 1 and len(lit_union) > 1:
                    self.codes[kind].append(auto_code(w, alpha, lit_union, rotate=1 + t % (len(lit_union) - 1) if t else 0))
                else:
                    self.codes[kind].append(auto_code(w, alpha, rec[kind][t].used))
        run(self)
        return self

    def _begin(self, blocks, npostfix, ndirect, modes, lit_map, dist_map, end):
        self.blk = [Blocks(b) for b in blocks]
        for b in self.blk:
            if b.n >= 2:
                b.left = BLOCK_BASE[b.first[0]] + b.first[1]
        self.npostfix, self.ndirect, self.end = npostfix, ndirect, end
        self.trace = [[0], [0], [0]]                       # the block types of each category in the order they came
        self.modes = list(modes) + [modes[-1]] * (self.blk[0].n - len(modes))
        self.cmap = [list(m["map"]) if m else None for m in (lit_map, dist_map)]
        self.ntrees = [lit_map["ntrees"] if lit_map else 1, self.blk[1].n, dist_map["ntrees"] if dist_map else 1]

    def _put_map(self, m):
        w = self.w
        varlen8(w, (m["ntrees"] if m else 1) - 1)
        if not m or m["ntrees"] < 2:
            return
        rlemax, imtf = m.get("rlemax", 0), m.get("imtf", 0)
        w.put(1 if rlemax else 0, 1)
        if rlemax:
            w.put(rlemax - 1, 4)
        syms = m.get("symbols") or map_symbols(mtf_encode(m["map"]) if imtf else list(m["map"]), rlemax)
        alpha = m["ntrees"] + rlemax
        make = m.get("code") or (lambda w_, a: auto_code(w_, a, {s for s, _ in syms}))
        code = make(w, alpha)
        for s, extra in syms:
            code.put(w, s)
            if 0 < s <= rlemax:
                w.put(extra, s)
        w.put(imtf, 1)

    def _switch(self, k):
        b, w = self.blk[k], self.w
        sym, count_code, extra = b.switches.pop(0)
        b.type_code_obj.put(w, sym)
        t = b.prev if sym == 0 else (b.type + 1 if sym == 1 else sym - 2)
        if t >= b.n:
            t -= b.n
        b.prev, b.type = b.type, t
        self.trace[k].append(t)
        b.count_code_obj.put(w, count_code)
        w.put(extra, BLOCK_EXTRA[count_code])
        b.left = BLOCK_BASE[count_code] + extra

    def _take(self, k):
        b = self.blk[k]
        if b.left == 0:
            self._switch(k)
        b.left -= 1
        return b.type

    def command(self, literals=b"", copy=2, dist=None, dcode=None, dextra=0, implicit=False, symbol=None, ins_extra=None, copy_extra=None, end=False):
        """One insert-and-copy command.  The distance: implicit (symbol below 128, the last distance), dcode + dextra as given, or `dist`, spelled without the ring.
        symbol / ins_extra / copy_extra override what literals and copy would choose (the bits written then no longer describe them: refused streams).
        end: the meta-block ends behind this command's literals (its copy length is written and never used)."""
        w = self.w
        literals = bytes(literals)
        ic, cc = length_code(INS_BASE, len(literals)), length_code(COPY_BASE, copy)
        sym = command_symbol(ic, cc, implicit) if symbol is None else symbol
        ic, cc, implicit = command_fields(sym)
        self.codes["I"][self._take(1)].put(w, sym)
        w.put(len(literals) - INS_BASE[ic] if ins_extra is None else ins_extra, INS_EXTRA[ic])
        w.put(copy - COPY_BASE[cc] if copy_extra is None else copy_extra, COPY_EXTRA[cc])
        L = self.blk[0]
        if self.ntrees[0] == 1 and L.left > len(literals) and len(literals) > 4096 and len(set(literals)) == 1:
            self.codes["L"][0].put(w, literals[0])                # (a long run of one byte under a code of one symbol: no bits)
            assert isinstance(self.codes["L"][0], Recorder) or self.codes["L"][0].single is not None
            L.left -= len(literals)
            self.out += literals
        else:
            for byte in literals:
                t = self._take(0)
                ctx = context_id(self.modes[t], self.p1, self.p2)
                self.contexts_met.add((self.modes[t], ctx))
                self.codes["L"][self.cmap[0][64 * t + ctx] if self.cmap[0] else 0].put(w, byte)
                self.out.append(byte)
        if end or len(self.out) >= self.end:
            return
        if implicit:
            dcode = 0
        else:
            if dcode is None:
                dcode, dextra = distance_code_for(dist, self.npostfix, self.ndirect)
            t = self._take(2)
            tree = self.cmap[1][4 * t + min(copy, 5) - 2] if self.cmap[1] else 0
            self.codes["D"][tree].put(w, dcode)
            w.put(dextra, distance_bits(dcode, self.npostfix, self.ndirect))
        d = distance_of(dcode, dextra, self.npostfix, self.ndirect, self.ring)
        self.last_distance = d
        self.distances.append(d)
        max_dist = min(len(self.out), self.max_back)
        if d <= 0:
            return
        if d > max_dist:                                          # section 8: a word of the static dictionary, transformed; it leaves the last distances alone
            self.uses_dictionary = True
            if not 4 <= copy <= 24 or self.dictionary is None:
                return
            ident = d - max_dist - 1
            index, t = ident & ((1 << NDBITS[copy]) - 1), ident >> NDBITS[copy]
            if t < 121:
                self.out += transform(dictionary_word(self.dictionary, copy, index), t)
            return
        if dcode != 0:
            self.ring = [d] + self.ring[:3]
        if d >= copy:
            self.out += self.out[len(self.out) - d:len(self.out) - d + copy]
        else:
            unit = bytes(self.out[-d:])
            self.out += (unit * (copy // d + 1))[:copy]

    def peek_distance(self, dcode, dextra=0):
        return distance_of(dcode, dextra, self.npostfix, self.ndirect, self.ring)

    def dictionary_distance(self, length, index, t):
        """the distance that names word `index` of `length` bytes under transform t at the current position"""
        return min(len(self.out), self.max_back) + 1 + ((t << NDBITS[length]) | index)

    def bytes(self):
        return self.w.bytes()
