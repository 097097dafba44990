"""Exact parses for the brotli encoder's block stage (tests/test_brotli_stages.py): a block is COMPOSED from literals and copies, which gives both the bytes and the parse.
`rows` turns the parse into the records the match finder would have left (gc_common.h GcSeqRaw: literals in front of the copy, offset << 8 | length, length at most 255 -- a
longer copy is a chain of records of one offset with no literals between them) and replays them to prove that they reproduce the bytes.  `merged` says which commands the
encoder has to make of them.  `Ring` is the decoder's ring of last distances (RFC 7932 section 4); `expected` walks a meta-block's commands with it and gives the distance
symbol the encoder is documented to choose ("Distance symbols"); `substitute` is the last-distance substitution as DESIGN.md describes it ("Substitution").
Nothing here is taken from the kernel: the models are written from those two texts and from the RFC."""
import numpy as np

import brotli_build as B

BLOCK_MAX = 1 << 17
MAX_SEQ = BLOCK_MAX // 5 + 8                                           # GC_MAX_SEQ_PER_BLOCK: entries of a row of the workspace
RING_WALK, SUB_MAX, TILE = 24, 512, 256


class Composer:
    """The content of one call, block by block.  lit(bytes) / copy(length, distance) append to the open block; end_block() closes it.  `blocks`: per block (start, length,
    [(ll, ml, off)]) -- the literals behind the last copy are the rest of the block."""
    def __init__(self):
        self.out, self.blocks, self.start, self.seqs, self.ll = bytearray(), [], 0, [], 0

    def lit(self, data):
        data = bytes(data)
        self.out += data
        self.ll += len(data)
        return self

    def copy(self, ml, off):
        n = len(self.out)
        assert 1 <= off <= n and ml >= 2, (ml, off, n)
        if off >= ml:
            self.out += self.out[n - off:n - off + ml]
        else:
            self.out += (bytes(self.out[n - off:]) * (ml // off + 1))[:ml]
        self.seqs.append((self.ll, ml, off))
        self.ll = 0
        return self

    def here(self):
        return len(self.out) - self.start                            # bytes in the open block

    def end_block(self, full=False):
        n = len(self.out) - self.start
        assert 0 < n <= BLOCK_MAX and (not full or n == BLOCK_MAX), n
        self.blocks.append((self.start, n, self.seqs))
        self.start, self.seqs, self.ll = len(self.out), [], 0
        return self

    def x(self):
        assert self.start == len(self.out), "a block is still open"
        assert all(n == BLOCK_MAX for _, n, _ in self.blocks[:-1]), "only the last block may be short"
        return np.frombuffer(bytes(self.out), dtype=np.uint8)


def split(ml, cap=255):
    """a copy as the lengths of its records: at most `cap` each, none shorter than 2"""
    out = []
    while ml > cap:
        take = cap if ml - cap >= 2 else ml - 2
        out.append(take)
        ml -= take
    out.append(ml)
    return out


def rows(x, blocks, cap=255):
    """blocks as Composer.blocks -> [(literals, records (k, 2) uint32)] for BrotliEncoder.code_parsed_device.  The records are replayed against x."""
    out = []
    for start, n, seqs in blocks:
        lits, recs, pos, rank = [], [], start, 0
        for ll, ml, off in seqs:
            lits.append(x[pos:pos + ll])
            pos += ll
            rank += ll
            for piece in split(ml, cap):
                recs.append((rank, (off << 8) | piece))
                pos += piece
        lits.append(x[pos:start + n])
        lit = np.concatenate(lits) if lits else np.zeros(0, np.uint8)
        rec = np.array(recs, dtype=np.uint32).reshape(-1, 2)
        replay(x, start, n, lit, rec)
        out.append((lit, rec))
    return out


def replay(x, start, n, lit, rec):
    """the block the records and literals stand for == x[start : start + n]"""
    lo = max(0, start - (int(rec[:, 1].max()) >> 8 if len(rec) else 0))
    got = bytearray(x[lo:start].tobytes())
    base, rank = len(got), 0
    for r, offml in rec.tolist():
        ml, off = offml & 255, offml >> 8
        got += lit[rank:r].tobytes()
        rank = r
        assert 2 <= ml and 1 <= off <= len(got), (ml, off, len(got))
        if off >= ml:
            got += got[len(got) - off:len(got) - off + ml]
        else:
            got += (bytes(got[len(got) - off:]) * (ml // off + 1))[:ml]
    got += lit[rank:].tobytes()
    assert len(got) - base == n and bytes(got[base:]) == x[start:start + n].tobytes(), "the parse does not reproduce the block"


def merged(seqs, n):
    """the commands of one block of n bytes as the encoder must form them: a copy with no literals and the distance of the one in front of it is part of that one; literals
    behind the last copy are an insert-only command (ll, 0, 0)"""
    out = []
    for ll, ml, off in seqs:
        if out and ll == 0 and off == out[-1][2]:
            out[-1] = (out[-1][0], out[-1][1] + ml, off)
        else:
            out.append((ll, ml, off))
    tail = n - sum(ll + ml for ll, ml, _ in out)
    assert tail >= 0
    return out + ([(tail, 0, 0)] if tail else [])


class Ring:
    """the decoder's last four distances, most recent first (RFC 7932 section 4): a stream starts with 4, 11, 15, 16; a distance is pushed unless its symbol was 0"""
    def __init__(self):
        self.r = [4, 11, 15, 16]

    def resolve(self, dsym, extra=0):
        return B.distance_of(dsym, extra, 0, 0, self.r)

    def push(self, d):
        self.r = [d] + self.r[:3]


SHORT = [(4, 0, -1), (5, 0, 1), (6, 0, -2), (7, 0, 2), (8, 0, -3), (9, 0, 3), (10, 1, -1), (11, 1, 1), (12, 1, -2), (13, 1, 2), (14, 1, -3), (15, 1, 3)]


def implicit_cell(ll, ml):
    return B.length_code(B.INS_BASE, ll) < 8 and (ml == 0 or B.length_code(B.COPY_BASE, ml) < 16)


def expected(cmds, ring):
    """cmds: [(ll, ml, dist)] of one meta-block -> [(ll, ml, dist, dsym)], dsym "implied", a distance symbol, or None behind an insert-only command; `ring` (the decoder's, as
    the meta-blocks in front left it) is moved along.  DESIGN.md "Distance symbols": symbol 0 where the distance is that of the command in front IN THIS META-BLOCK; otherwise
    the encoder may name ring entry 0 (the command in front) and every older entry whose run ends among the RING_WALK commands in front of the command, in the order of
    preference 1, 2, 3, then entry 0 -1 +1 -2 +2 -3 +3 (4 .. 9), then entry 1 likewise (10 .. 15); otherwise the explicit code."""
    out = []
    for j, (ll, ml, d) in enumerate(cmds):
        if ml == 0:
            out.append((ll, 0, 0, None))
            continue
        if j and d == cmds[j - 1][2]:
            out.append((ll, ml, d, "implied" if implicit_cell(ll, ml) else 0))
            continue
        known = 0
        if j:                                                          # how many entries the encoder knows: changes of distance among commands j - 1 .. j - RING_WALK
            known, cur = 1, cmds[j - 1][2]
            for k in range(j - 2, max(-1, j - 1 - RING_WALK), -1):
                if known == 4:
                    break
                if cmds[k][2] != cur:
                    cur = cmds[k][2]
                    assert ring.r[known] == cur, "the walk's entry is not the decoder's"
                    known += 1
        sym = None
        for code in (1, 2, 3):
            if sym is None and known > code and d == ring.r[code]:
                sym = code
        for code, entry, delta in SHORT:
            if sym is None and known > entry and d == ring.r[entry] + delta:
                sym = code
        if sym is None:
            sym = B.distance_code_for(d, 0, 0)[0]
        out.append((ll, ml, d, sym))
        ring.push(d)
    return out


def substitute(x, start, cmds, passes):
    """DESIGN.md "Substitution": per pass and per tile of TILE commands, first every command of the tile decides on the distances as they stand, then the tile's decisions
    are stored.  A copy (not the first command) of at most SUB_MAX bytes whose distance differs from the command's in front looks at the distances of the up to three
    commands in front, nearest first, stops at one that is its own distance, and takes the first at which the same bytes stand."""
    cmds = [list(c) for c in cmds]
    xb = x.tobytes() if hasattr(x, "tobytes") else bytes(x)
    ncopy = len(cmds) - (1 if cmds and cmds[-1][1] == 0 else 0)
    at, pos = [], start
    for ll, ml, _ in cmds:
        at.append(pos + ll)
        pos += ll + ml
    for _ in range(passes):
        for tb in range(0, ncopy, TILE):
            new = {}
            for j in range(max(tb, 1), min(tb + TILE, ncopy)):
                ll, ml, off = cmds[j]
                if cmds[j - 1][2] == off or ml > SUB_MAX:
                    continue
                for k in range(1, min(3, j) + 1):
                    dk = cmds[j - k][2]
                    if dk == off:
                        break
                    if xb[at[j] - dk:at[j] - dk + ml] == xb[at[j]:at[j] + ml]:
                        new[j] = dk
                        break
            for j, dk in new.items():
                cmds[j][2] = dk
    return [tuple(c) for c in cmds]
