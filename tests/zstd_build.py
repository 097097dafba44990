"""A zstd frame builder that is also the model of what a decoder must produce, written from RFC 8878 (section numbers in the comments are the RFC's).  It writes exactly
what it is told to write, valid or not: the hand-built frames of tests/test_zstd_dec_handmade.py come from here, and so do the frames no decoder may accept.

    FwdBits / BackBits              forward (LSB first, 4.1.1) and backward (4.1 / 4.2.2: read from the end, below an end mark) bit streams
    ncount / FseTable               an FSE table description from an explicit normalised distribution, and the decoding table it stands for; FseTable finds the
                                    states an encoder has to go through (the decoder's walk backwards)
    Huffman                         prefix codes from explicit weights (4.2.1); direct and FSE-compressed weight descriptions (two interleaved states); streams
    lit_raw / lit_rle / lit_huf     the literals section, every size format, one or four streams
    nseq_bytes / seq_codes          sequence counts in every encoding; (literal length, match length, offset value) -> codes and extra bits
    frame_header / block_header     every field explicit
    Frame                           blocks of a frame; its state is the model: the content, the three repeat offsets, the tables and the tree a later block may repeat
    xxh64                           the content checksum in plain Python

The predefined distributions (3.1.1.3.2.2) and the baseline tables (3.1.1.3.2.1.1) are typed in from the RFC."""
import struct

MAGIC = 0xFD2FB528
BLOCK_MAX = 1 << 17
LL, OF, ML = 0, 1, 2                                                                                       # the order of the descriptions in a sequences section
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEFAULT = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_DEFAULT = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)
assert len(LL_BASE) == len(LL_BITS) == len(LL_DEFAULT[0]) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DEFAULT[0]) == 53 and len(OF_DEFAULT[0]) == 29
DEFAULTS = {LL: LL_DEFAULT, OF: OF_DEFAULT, ML: ML_DEFAULT}
MODE_PREDEFINED, MODE_RLE, MODE_FSE, MODE_REPEAT = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------- bits
class FwdBits:
    """LSB-first bits, read in the order written"""
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits), (value, bits)
        self.acc |= value << self.n
        self.n += bits

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


class BackBits:
    """A stream the decoder reads from its end: `read(value, bits)` records what the decoder is to read next, in ITS order; bytes() writes the fields last-read first,
    then the end mark (a 1 bit) and zeros up to the byte."""
    def __init__(self):
        self.reads = []

    def read(self, value, bits):
        assert 0 <= value < (1 << bits), (value, bits)
        self.reads.append((value, bits))

    @property
    def nbits(self):
        return sum(b for _, b in self.reads)

    def bytes(self, mark=True):
        w = FwdBits()
        for value, bits in reversed(self.reads):
            w.put(value, bits)
        if mark:
            w.put(1, 1)
        return w.bytes()


def hibit(v):
    return v.bit_length() - 1


# ---------------------------------------------------------------------------------------------- FSE (4.1.1)
def ncount(norm, log, log_field=None):
    """the description of a normalised distribution (counts; -1 = "less than one"); every symbol of `norm` is written, whatever the counts add up to"""
    w = FwdBits()
    w.put(log - 5 if log_field is None else log_field, 4)
    norm = list(norm)
    while norm and norm[-1] == 0:                                   # (the symbols behind the last one with a count have no description)
        norm.pop()
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    s = 0
    while s < len(norm):
        count = norm[s]
        v = count + 1
        mx = (2 * threshold - 1) - remaining
        if v < mx:
            w.put(v, nbits - 1)
        elif v < threshold:
            w.put(v, nbits)
        else:
            w.put(v + mx, nbits)
        remaining -= abs(count)
        s += 1
        while remaining < threshold and threshold > 1:
            nbits -= 1
            threshold >>= 1
        if count == 0:                                              # a repeat flag follows every zero: how many more zeros, 3 = "three, and another flag"
            run = 0
            while s + run < len(norm) and norm[s + run] == 0:
                run += 1
            s += run
            while run >= 3:
                w.put(3, 2)
                run -= 3
            w.put(run, 2)
    return w.bytes()


class FseTable:
    """the decoding table of a distribution: sym / nb / base per state"""
    def __init__(self, norm, log):
        size = 1 << log
        assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
        self.log, self.norm = log, list(norm)
        cell = [None] * size
        high = size - 1
        for s, c in enumerate(norm):                                # "less than one" symbols take the last cells, the first of them the very last
            if c == -1:
                cell[high] = s
                high -= 1
        pos, step = 0, (size >> 1) + (size >> 3) + 3
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                cell[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0
        nxt = [max(abs(c), 0) for c in norm]
        self.sym, self.nb, self.base = cell, [0] * size, [0] * size
        for u in range(size):
            s = cell[u]
            n = nxt[s]
            nxt[s] += 1
            self.nb[u] = log - hibit(n)
            self.base[u] = (n << self.nb[u]) - size
        self.rle = False

    @classmethod
    def of_rle(cls, sym):
        t = cls.__new__(cls)
        t.log, t.sym, t.nb, t.base, t.rle, t.norm = 0, [sym], [0], [0], True, None
        return t

    def states(self, sym):
        return [u for u, s in enumerate(self.sym) if s == sym]

    def last_state(self, sym, most_bits=True):
        """a state for the symbol nothing follows: the one whose update reads the most (or the fewest) bits"""
        c = self.states(sym)
        assert c, "symbol %d has no state" % sym
        return (max if most_bits else min)(c, key=lambda u: (self.nb[u], -u if most_bits else u))

    def before(self, sym, nxt):
        """the state that emits `sym` and can move on to state `nxt` -> (state, bits value, bits)"""
        for u in self.states(sym):
            if self.base[u] <= nxt < self.base[u] + (1 << self.nb[u]):
                return u, nxt - self.base[u], self.nb[u]
        raise AssertionError("symbol %d has no state in front of state %d" % (sym, nxt))


def fse_walk(table, symbols, last=None):
    """the states a decoder goes through to emit `symbols` -> (states, [(value, bits)] of the update behind every symbol but the last)"""
    if not symbols:
        return [], []
    states = [table.last_state(symbols[-1]) if last is None else last]
    moves = []
    for s in reversed(symbols[:-1]):
        u, v, nb = table.before(s, states[0])
        states.insert(0, u)
        moves.insert(0, (v, nb))
    return states, moves


# ---------------------------------------------------------------------------------------------- Huffman (4.2)
def huf_direct(weights):
    """header byte 127 + n, then n weights of 4 bits (the last weight of the tree is implied and not in the list)"""
    w = list(weights) + [0] * (len(weights) & 1)
    return bytes([127 + len(weights)]) + bytes((w[i] << 4) | w[i + 1] for i in range(0, len(w), 2))


def huf_fse(weights, norm, log, log_field=None, size_byte=None):
    """weights (without the implied last one) FSE-compressed with two interleaved states: the decoder takes weight 0 from state 1, weight 1 from state 2, ... and, when a
    state's update reads past the start of the stream, the other state's symbol as the last weight"""
    t = FseTable(norm, log)
    chain = [fse_walk(t, list(weights[k::2])) for k in (0, 1)]
    r = BackBits()
    r.read(chain[0][0][0], log)
    r.read(chain[1][0][0], log)
    for i in range(len(weights) - 2):
        r.read(*chain[i & 1][1][i >> 1])
    over = chain[len(weights) & 1][0][-1]                          # the state behind the last weight but one: its update must over-read
    assert t.nb[over] > 0, "the last update reads no bits: the decoder would not see the end"
    body = ncount(norm, log, log_field) + r.bytes()
    return bytes([len(body) if size_byte is None else size_byte]) + body


class Huffman:
    """codes from the weights of symbols 0..n-1 (the last one included; it must be the one the others imply)"""
    def __init__(self, weights):
        self.weights = list(weights)
        total = sum(1 << (w - 1) for w in weights if w)
        self.log = hibit(total)
        assert total == 1 << self.log, "the weights do not complete a power of two"
        rest = (1 << self.log) - sum(1 << (w - 1) for w in weights[:-1] if w)
        assert weights[-1] and rest == 1 << (weights[-1] - 1), "the last weight is not the implied one"
        self.code = {}
        pos = 0
        for w in range(1, self.log + 1):                             # the lowest weights (longest codes) first, symbols in order: consecutive code values
            for s, ws in enumerate(weights):
                if ws == w:
                    self.code[s] = (pos >> (w - 1), self.log + 1 - w)
                    pos += 1 << (w - 1)

    def direct(self):
        return huf_direct(self.weights[:-1])

    def fse(self, norm, log):
        return huf_fse(self.weights[:-1], norm, log)

    def stream(self, data):
        r = BackBits()
        for b in data:
            r.read(*self.code[b])
        return r.bytes()

    def stream_bits(self, data):
        return sum(self.code[b][1] for b in data)


def four_streams(huf, data, jump=None):
    seg = (len(data) + 3) // 4
    parts = [huf.stream(data[i * seg:(i + 1) * seg]) for i in range(4)]                                   # (a stream of no symbols is its end mark)
    sizes = [len(p) for p in parts[:3]] if jump is None else jump
    return struct.pack("<HHH", *sizes) + b"".join(parts)


# ---------------------------------------------------------------------------------------------- literals section (3.1.1.3.1)
def lit_header_plain(ltype, size, form):
    """raw (0) / RLE (1) literals: form 1, 2 or 3 = bytes of the header; form 1 may also use size-format bits 10 (form="1b")"""
    if form in (1, "1b"):
        assert size < 32
        return bytes([ltype | ((0 if form == 1 else 2) << 2) | (size << 3)])
    if form == 2:
        assert size < 4096
        return struct.pack("<H", ltype | (1 << 2) | (size << 4))
    assert size < (1 << 20)
    return struct.pack("<I", ltype | (3 << 2) | (size << 4))[:3]


def lit_raw(data, form=None):
    form = form or (1 if len(data) < 32 else 2 if len(data) < 4096 else 3)
    return lit_header_plain(0, len(data), form) + bytes(data)


def lit_rle(byte, n, form=None):
    form = form or (1 if n < 32 else 2 if n < 4096 else 3)
    return lit_header_plain(1, n, form) + bytes([byte])


def lit_header_huf(ltype, form, regen, comp):
    """compressed (2) / treeless (3) literals: size format 0 (one stream, 10 + 10 bits), 1 (four streams, 10 + 10), 2 (14 + 14), 3 (18 + 18)"""
    bits = (10, 10, 14, 18)[form]
    assert regen < (1 << bits) and comp < (1 << bits), (regen, comp, form)
    v = ltype | (form << 2) | (regen << 4) | (comp << (4 + bits))
    return v.to_bytes((3, 3, 4, 5)[form], "little")


def lit_huf(huf, data, form, tree=None, treeless=False, payload=None, regen=None, comp=None):
    """tree: the description's bytes (default: direct weights); payload: the stream bytes instead of the encoded `data`"""
    desc = b"" if treeless else (huf.direct() if tree is None else tree)
    if payload is None:
        payload = huf.stream(data) if form == 0 else four_streams(huf, data)
    body = desc + payload
    return lit_header_huf(3 if treeless else 2, form, len(data) if regen is None else regen, len(body) if comp is None else comp) + body


# ---------------------------------------------------------------------------------------------- sequences section (3.1.1.3.2)
def nseq_bytes(n, form=None):
    form = form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert 0 <= n - 0x7F00 < 65536
    return b"\xff" + struct.pack("<H", n - 0x7F00)


def ll_code(ll):
    c = max(i for i in range(36) if LL_BASE[i] <= ll)
    assert ll - LL_BASE[c] < (1 << LL_BITS[c])
    return c, ll - LL_BASE[c]


def ml_code(ml):
    c = max(i for i in range(53) if ML_BASE[i] <= ml)
    assert ml - ML_BASE[c] < (1 << ML_BITS[c])
    return c, ml - ML_BASE[c]


def of_code(value):
    """Offset_Value (1..3: a repeat offset; offset + 3 otherwise) -> code, extra bits"""
    c = hibit(value)
    return c, value - (1 << c)


def seq_codes(ll, ml, ofv):
    return ll_code(ll) + of_code(ofv) + ml_code(ml)               # (llc, llx, ofc, ofx, mlc, mlx)


def seq_values(c):
    llc, llx, ofc, ofx, mlc, mlx = c
    return LL_BASE[llc] + llx, ML_BASE[mlc] + mlx, (1 << ofc) + ofx


def seq_bitstream(codes, tables, last_states=None):
    """the backward bitstream of sequences given as codes and extra bits, under the three decoding tables -> BackBits"""
    walks = [fse_walk(tables[w], [c[2 * w] for c in codes], None if last_states is None else last_states[w]) for w in (LL, OF, ML)]
    r = BackBits()
    for w in (LL, OF, ML):
        r.read(walks[w][0][0], tables[w].log)
    for i, c in enumerate(codes):
        r.read(c[3], c[2])                                          # offset: as many extra bits as the code says
        r.read(c[5], ML_BITS[c[4]])
        r.read(c[1], LL_BITS[c[0]])
        if i + 1 < len(codes):
            for w in (LL, ML, OF):
                r.read(*walks[w][1][i])
    return r


# ---------------------------------------------------------------------------------------------- frame and blocks (3.1.1)
def frame_header(fcs=None, fcs_bytes=None, single=False, window=None, did=0, did_bytes=0, checksum=False, reserved=0, unused=0, magic=MAGIC):
    """fcs_bytes: 0, 1 (needs single), 2 (the field holds fcs - 256), 4, 8; window: the descriptor byte (absent with single)"""
    if fcs_bytes is None:
        fcs_bytes = 0 if fcs is None else (1 if single and fcs < 256 else 2 if 256 <= fcs < 65792 else 4 if fcs < (1 << 32) else 8)
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    assert (fcs_bytes == 1) <= single and (fcs_bytes != 0 or not single)
    out = struct.pack("<I", magic) + bytes([(flag << 6) | (single << 5) | (unused << 4) | (reserved << 3) | (checksum << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]])
    if not single:
        out += bytes([0 if window is None else window])
    out += did.to_bytes(did_bytes, "little")
    if fcs_bytes:
        out += (fcs - 256 if fcs_bytes == 2 else fcs).to_bytes(fcs_bytes, "little")
    return out


def block_header(last, btype, size):
    return struct.pack("<I", int(last) | (btype << 1) | (size << 3))[:3]


def dist(n, counts):
    """a distribution over n symbols from {symbol: count}"""
    out = [0] * n
    for s, c in counts.items():
        out[s] = c
    return out


def skippable(nibble, data=b""):
    return struct.pack("<II", 0x184D2A50 | nibble, len(data)) + bytes(data)


def resolve(rep, ofv, ll):
    """3.1.1.5: an offset value and the repeat offsets in front of the sequence -> (offset, the repeat offsets behind it)"""
    if ofv > 3:
        return ofv - 3, [ofv - 3, rep[0], rep[1]]
    idx = ofv - 1 + (ll == 0)
    off = rep[idx] if idx < 3 else rep[0] - 1
    if idx == 0:
        return off, list(rep)
    return off, ([off, rep[0], rep[2]] if idx == 1 else [off, rep[0], rep[1]])


class Frame:
    """The blocks of one frame, and the model.  out: the content; rep: the repeat offsets; tables / huf: what Repeat_Mode and treeless literals refer to.  `sound` turns
    False when a sequence asks for what a decoder has to refuse."""
    def __init__(self):
        self.body, self.out, self.rep, self.tables, self.huf, self.sound = bytearray(), bytearray(), [1, 4, 8], [None, None, None], None, True
        self.reps = []                                              # the repeat offsets behind every block

    def raw(self, data, last=False, size=None):
        self.body += block_header(last, 0, len(data) if size is None else size) + bytes(data)
        self.out += bytes(data)
        self.reps.append(tuple(self.rep))

    def rle(self, byte, n, last=False):
        self.body += block_header(last, 1, n) + bytes([byte])
        self.out += bytes([byte]) * n
        self.reps.append(tuple(self.rep))

    def bare(self, btype, payload, last=False, size=None):
        """a block whose payload the model knows nothing about"""
        self.body += block_header(last, btype, len(payload) if size is None else size) + bytes(payload)
        self.sound = False

    def execute(self, literals, seqs):
        """3.1.1.4, 3.1.1.5: seqs = (literal length, match length, offset value)"""
        lp = 0
        start = len(self.out)
        for ll, ml, ofv in seqs:
            if lp + ll > len(literals):
                self.sound = False
            self.out += literals[lp:lp + ll]
            lp += ll
            off, self.rep = resolve(self.rep, ofv, ll)
            if off <= 0 or off > len(self.out):
                self.sound = False
                off = 1 if not self.out else min(max(off, 1), len(self.out))
                if not self.out:
                    self.out += b"\0"
            if off >= ml:
                self.out += self.out[len(self.out) - off:len(self.out) - off + ml]
            else:
                piece = bytes(self.out[len(self.out) - off:])
                self.out += (piece * (ml // off + 1))[:ml]
        self.out += literals[lp:]
        if len(self.out) - start > BLOCK_MAX:
            self.sound = False

    def compressed(self, lit, literals, seqs=(), modes=(MODE_PREDEFINED,) * 3, specs=(None, None, None), last=False, nseq_form=None, nseq=None, reserved=0, huf=None,
                   codes=None, tail=b"", pad_to=None, last_states=None, mark=True):
        """lit: the literals section; literals: what it regenerates; seqs: (ll, ml, offset value) or, with `codes`, (llc, llx, ofc, ofx, mlc, mlx) each.
        modes / specs per table in the order LL, OF, ML: RLE -> the symbol, FSE -> (norm, log) [or (norm, log, description bytes)], repeat / predefined -> None.
        huf: the tree this block's literals section describes (treeless blocks behind it use it)."""
        cs = list(codes) if codes is not None else [seq_codes(*s) for s in seqs]
        seqs = [seq_values(c) for c in cs]
        n = len(cs)
        payload = bytearray(lit) + nseq_bytes(n if nseq is None else nseq, nseq_form)
        if n or nseq:
            payload.append((modes[LL] << 6) | (modes[OF] << 4) | (modes[ML] << 2) | reserved)
            tabs = []
            for w in (LL, OF, ML):
                m, spec = modes[w], specs[w]
                if m == MODE_PREDEFINED:
                    t = FseTable(*DEFAULTS[w])
                elif m == MODE_RLE:
                    payload.append(spec)
                    t = FseTable.of_rle(spec)
                elif m == MODE_FSE:
                    payload += spec[2] if len(spec) > 2 else ncount(spec[0], spec[1])
                    t = FseTable(spec[0], spec[1])
                else:
                    t = self.tables[w]
                    if t is None:                                   # nothing to repeat: no decoder gets as far as the bitstream
                        t, self.sound = FseTable(*DEFAULTS[w]), False
                tabs.append(t)
            if n:
                self.tables = tabs
                payload += seq_bitstream(cs, tabs, last_states).bytes(mark)
        payload += tail
        if huf is not None:
            self.huf = huf
        self.body += block_header(last, 2, len(payload)) + payload
        self.execute(bytes(literals), seqs)
        self.reps.append(tuple(self.rep))
        return len(payload)

    def bytes(self, header=None, checksum_value=None, **kw):
        """header: bytes, or None for frame_header(**kw); a checksum flag in kw appends XXH64's low 4 bytes (checksum_value: this value instead)"""
        h = frame_header(**kw) if header is None else header
        out = h + bytes(self.body)
        if kw.get("checksum") or checksum_value is not None:
            out += struct.pack("<I", (xxh64(bytes(self.out)) & 0xFFFFFFFF) if checksum_value is None else checksum_value)
        return out


# ---------------------------------------------------------------------------------------------- XXH64 (seed 0)
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
_M = (1 << 64) - 1


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & _M


def _round(acc, lane):
    return (_rotl((acc + lane * _P2) & _M, 31) * _P1) & _M


def xxh64(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while p + 32 <= n:
            for i in range(4):
                v[i] = _round(v[i], int.from_bytes(data[p + 8 * i:p + 8 * i + 8], "little"))
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for i in range(4):
            h = ((h ^ _round(0, v[i])) * _P1 + _P4) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & _M), 11) * _P1) & _M
        p += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    return h ^ (h >> 32)
