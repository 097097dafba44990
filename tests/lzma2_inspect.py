"""An LZMA2 stream reader for the encoder tests (tests/test_lzma2_stages.py), written from the format's description -- the LZMA2 chunk layer (control byte, sizes, props
byte, the reset rules), the LZMA range decoder, the 12-state machine, the literal / match / repeat grammar, the length and distance coders -- and from nothing in this
project: neither the encoder's kernels nor the decoder port.  It says what an encoder WROTE: per chunk the control byte, the props, both sizes and every symbol with its
position, kind, length, distance and the coder state in front of it.

It insists on what a conforming LZMA2 decoder insists on: the first chunk resets the dictionary; the first LZMA chunk behind a dictionary reset resets the state and carries
props; control bytes 3..0x7F do not exist; lc + lp <= 4; the first byte of a chunk's range-coder data is 0; a distance reaches no further back than the dictionary holds (or
than the stated dictionary size); no end-of-payload marker; a chunk produces exactly its unpacked size from exactly its packed size, and the range decoder is at rest behind
it (code == 0); the stream ends with a 0x00 control byte unless the caller says it need not."""
from collections import namedtuple

LIT, MLIT, MATCH, SHORTREP, REP0, REP1, REP2, REP3 = "literal", "matched literal", "match", "short rep", "rep0", "rep1", "rep2", "rep3"
REP_KINDS = (REP0, REP1, REP2, REP3)

Symbol = namedtuple("Symbol", "pos kind length dist state")          # pos: in the content; dist: 1-based (0 for a plain literal); state: before the symbol
Chunk = namedtuple("Chunk", "control props usize csize pos symbols")  # props: (lc, lp, pb) in force, None for a stored chunk; symbols: [] for a stored chunk
Stream = namedtuple("Stream", "chunks content end_mark")


class FormatError(ValueError):
    pass


class _Rc:
    """the range decoder over data[at : at + n]"""
    def __init__(self, data, at, n):
        if n < 5:
            raise FormatError("an LZMA chunk of fewer than 5 packed bytes")
        if data[at] != 0:
            raise FormatError("the first byte of the range coder's data is not 0")
        self.d, self.at, self.end = data, at + 5, at + n
        self.range, self.code = 0xFFFFFFFF, int.from_bytes(data[at + 1:at + 5], "big")

    def _norm(self):
        if self.range < (1 << 24):
            if self.at >= self.end:
                raise FormatError("the range decoder reads behind the chunk's packed size")
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.code = ((self.code << 8) | self.d[self.at]) & 0xFFFFFFFF
            self.at += 1

    def bit(self, probs, i):
        p = probs[i]
        bound = (self.range >> 11) * p
        if self.code < bound:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
            b = 0
        else:
            self.range -= bound
            self.code -= bound
            probs[i] = p - (p >> 5)
            b = 1
        self._norm()
        return b

    def direct(self, n):
        v = 0
        for _ in range(n):
            self.range >>= 1
            b = 1 if self.code >= self.range else 0
            if b:
                self.code -= self.range
            v = (v << 1) | b
            self._norm()
        return v

    def tree(self, probs, base, nbits):
        m = 1
        for _ in range(nbits):
            m = (m << 1) | self.bit(probs, base + m)
        return m - (1 << nbits)

    def tree_rev(self, probs, base, nbits):
        m, v = 1, 0
        for i in range(nbits):
            b = self.bit(probs, base + m)
            m = (m << 1) | b
            v |= b << i
        return v


class _Model:
    """the adaptive probabilities, one flat list per table, all 1024 after a state reset"""
    def __init__(self, lc, lp):
        h = lambda n: [1024] * n
        self.is_match, self.is_rep, self.g0, self.g1, self.g2, self.rep0_long = h(12 * 16), h(12), h(12), h(12), h(12), h(12 * 16)
        self.len, self.rep_len = self._len(), self._len()
        self.slot, self.spec, self.align = h(4 * 64), h(115 + 64), h(16)
        self.lit = h(0x300 << (lc + lp))

    @staticmethod
    def _len():
        return {"choice": [1024, 1024], "low": [1024] * (16 * 8), "mid": [1024] * (16 * 8), "high": [1024] * 256}


def _length(rc, t, pos_state):
    if rc.bit(t["choice"], 0) == 0:
        return 2 + rc.tree(t["low"], pos_state * 8, 3)
    if rc.bit(t["choice"], 1) == 0:
        return 10 + rc.tree(t["mid"], pos_state * 8, 3)
    return 18 + rc.tree(t["high"], 0, 8)


def inspect(data, dict_size=None, need_end_mark=True):
    """bytes of an LZMA2 stream -> Stream(chunks, content, end_mark)"""
    data = bytes(data)
    out = bytearray()
    chunks, at = [], 0
    need = 0xE0                              # the least LZMA control byte the next LZMA chunk may have (0xE0: nothing seen yet; 0xC0: behind a dictionary reset; 0: any)
    dict_base = 0                            # where the dictionary starts in `out`
    props = model = None
    state, reps = 0, [0, 0, 0, 0]            # reps: distance - 1
    pending = 0                              # bytes of a match that the previous chunk's end cut off (copied at reps[0])
    end_mark = False
    while at < len(data):
        control = data[at]
        if control == 0:
            end_mark = True
            at += 1
            break
        if control < 0x80:
            if control > 2:
                raise FormatError("control byte 0x%02X does not exist" % control)
            if at + 3 > len(data):
                raise FormatError("a stored chunk's header is cut off")
            n = int.from_bytes(data[at + 1:at + 3], "big") + 1
            if control == 1:
                need, dict_base = 0xC0, len(out)
            elif need == 0xE0:
                raise FormatError("the first chunk does not reset the dictionary")
            if pending:
                raise FormatError("a stored chunk inside a match")
            if at + 3 + n > len(data):
                raise FormatError("a stored chunk is cut off")
            chunks.append(Chunk(control, None, n, n, len(out), []))
            out += data[at + 3:at + 3 + n]
            at += 3 + n
            continue
        if control < need:
            raise FormatError("control byte 0x%02X where at least 0x%02X is needed" % (control, need))
        need = 0
        mode = (control >> 5) & 3
        hdr = 6 if mode >= 2 else 5
        if at + hdr > len(data):
            raise FormatError("an LZMA chunk's header is cut off")
        usize = ((control & 0x1F) << 16) + int.from_bytes(data[at + 1:at + 3], "big") + 1
        csize = int.from_bytes(data[at + 3:at + 5], "big") + 1
        if mode == 3:
            dict_base = len(out)
        if mode >= 2:
            pbyte = data[at + 5]
            if pbyte >= 9 * 5 * 5:
                raise FormatError("props byte 0x%02X" % pbyte)
            lc, lp, pb = pbyte % 9, (pbyte // 9) % 5, pbyte // 45
            if lc + lp > 4:
                raise FormatError("lc + lp > 4")
            props = (lc, lp, pb)
        if mode >= 1:
            if pending:
                raise FormatError("a state reset inside a match")
            model, state, reps = _Model(props[0], props[1]), 0, [0, 0, 0, 0]
        if at + hdr + csize > len(data):
            raise FormatError("an LZMA chunk is cut off")
        lc, lp, pb = props
        rc = _Rc(data, at + hdr, csize)
        start, end, syms = len(out), len(out) + usize, []
        if pending:
            k = min(pending, usize)
            for _ in range(k):
                out.append(out[len(out) - reps[0] - 1])
            pending -= k
        while len(out) < end:
            pos = len(out)
            ppos = pos - dict_base                                   # the decoder's processedPos: position since the dictionary reset
            ps = ppos & ((1 << pb) - 1)
            if rc.bit(model.is_match, state * 16 + ps) == 0:
                prev = out[pos - 1] if ppos else 0
                base = 0x300 * (((ppos & ((1 << lp) - 1)) << lc) + (prev >> (8 - lc)))
                if state < 7:
                    sym = 1
                    while sym < 0x100:
                        sym = (sym << 1) | rc.bit(model.lit, base + sym)
                    syms.append(Symbol(pos, LIT, 1, 0, state))
                else:
                    if reps[0] >= ppos:
                        raise FormatError("a matched literal whose distance reaches in front of the dictionary")
                    mb, sym, offs = out[pos - reps[0] - 1], 1, 0x100
                    while sym < 0x100:
                        mb <<= 1
                        bit_m = mb & offs
                        b = rc.bit(model.lit, base + offs + bit_m + sym)
                        sym = (sym << 1) | b
                        offs &= (~bit_m if b == 0 else bit_m) & 0x1FF
                    syms.append(Symbol(pos, MLIT, 1, reps[0] + 1, state))
                out.append(sym & 0xFF)
                state = 0 if state < 4 else (state - 3 if state < 10 else state - 6)
                continue
            if rc.bit(model.is_rep, state) == 0:
                length = _length(rc, model.len, ps)
                slot = rc.tree(model.slot, min(length - 2, 3) * 64, 6)
                if slot < 4:
                    dist = slot
                else:
                    nb = (slot >> 1) - 1
                    dist = (2 | (slot & 1)) << nb
                    if slot < 14:
                        dist += rc.tree_rev(model.spec, dist - slot - 1, nb)      # the reverse trees of slots 4..13 share one array: this slot's tree starts at base - slot - 1
                    else:
                        dist += rc.direct(nb - 4) << 4
                        dist += rc.tree_rev(model.align, 0, 4)
                if dist == 0xFFFFFFFF:
                    raise FormatError("an end-of-payload marker, which LZMA2 does not have")
                reps = [dist, reps[0], reps[1], reps[2]]
                kind, st_after = MATCH, (7 if state < 7 else 10)
            else:
                if rc.bit(model.g0, state) == 0:
                    if rc.bit(model.rep0_long, state * 16 + ps) == 0:
                        if reps[0] >= ppos:
                            raise FormatError("a short rep whose distance reaches in front of the dictionary")
                        syms.append(Symbol(pos, SHORTREP, 1, reps[0] + 1, state))
                        out.append(out[pos - reps[0] - 1])
                        state = 9 if state < 7 else 11
                        continue
                    kind = REP0
                else:
                    if rc.bit(model.g1, state) == 0:
                        kind, d = REP1, reps[1]
                        reps = [d, reps[0], reps[2], reps[3]]
                    elif rc.bit(model.g2, state) == 0:
                        kind, d = REP2, reps[2]
                        reps = [d, reps[0], reps[1], reps[3]]
                    else:
                        kind, d = REP3, reps[3]
                        reps = [d, reps[0], reps[1], reps[2]]
                length = _length(rc, model.rep_len, ps)
                st_after = 8 if state < 7 else 11
            if reps[0] >= ppos or (dict_size is not None and reps[0] >= dict_size):
                raise FormatError("a distance of %d at position %d reaches in front of the dictionary" % (reps[0] + 1, pos))
            syms.append(Symbol(pos, kind, length, reps[0] + 1, state))
            state = st_after
            k = min(length, end - pos)
            pending = length - k
            for _ in range(k):
                out.append(out[len(out) - reps[0] - 1])
        if rc.at != rc.end:
            raise FormatError("an LZMA chunk leaves %d of its packed bytes unread" % (rc.end - rc.at))
        if rc.code != 0:
            raise FormatError("the range decoder is not at rest at the chunk's end")
        chunks.append(Chunk(control, props, usize, csize, start, syms))
        at += hdr + csize
    if pending:
        raise FormatError("the stream ends inside a match")
    if need_end_mark and not end_mark:
        raise FormatError("no end marker")
    if at != len(data):
        raise FormatError("%d bytes behind the end marker" % (len(data) - at))
    return Stream(chunks, bytes(out), end_mark)


def symbols(stream):
    return [s for c in stream.chunks for s in c.symbols]
