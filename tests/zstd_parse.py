"""Exact parses for the zstd encoder's entropy stage (tests/test_zstd_entropy.py): a block is COMPOSED from literals and matches, which gives both the bytes and the parse;
`rows` turns the parse into the records the match finder would have left (gc_common.h GcSeqRaw: literals in front of the match, offset << 8 | length, length at most 255 --
a longer match is a chain of records of one offset with no literals between them) and replays the records to prove that they reproduce the bytes; `merged` says which
sequences the encoder has to make of them (K3a joins a record to the one in front of it when it has the same offset and no literals: chains, and whatever else looks like one)."""
import numpy as np

BLOCK_MAX = 1 << 17


class Composer:
    """The content of one frame, block by block.  lit(bytes) / match(ml, off) append to the open block; end_block() closes it.  `blocks`: per block (start, length,
    [(ll, ml, off)]) -- the literals behind the last match are the rest of the block."""
    def __init__(self):
        self.out, self.blocks, self.start, self.seqs, self.ll = bytearray(), [], 0, [], 0

    def lit(self, data):
        data = bytes(data)
        self.out += data
        self.ll += len(data)
        return self

    def match(self, ml, off):
        n = len(self.out)
        assert 1 <= off <= n, (off, n)
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


def split(ml, cap):
    """a match as the lengths of its records: at most `cap` each, none shorter than 3"""
    assert ml >= 3 and 6 <= cap <= 255
    out = []
    while ml > cap:
        take = cap if ml - cap >= 3 else ml - 3
        out.append(take)
        ml -= take
    out.append(ml)
    return out


def rows(x, blocks, cap=255, frame_start=0):
    """blocks as Composer.blocks -> [(literals, records (k, 2) uint32)] for ZstdEncoder.code_parsed_device.  cap: an int, or a function of (block, sequence) -> int, so that a
    test chooses where a chain breaks.  The records are replayed against x (offsets reach back to frame_start at most)."""
    out = []
    for b, (start, n, seqs) in enumerate(blocks):
        lits, recs, pos, rank = [], [], start, 0
        for i, (ll, ml, off) in enumerate(seqs):
            lits.append(x[pos:pos + ll])
            pos += ll
            rank += ll
            for piece in split(ml, cap(b, i) if callable(cap) else cap):
                recs.append((rank, (off << 8) | piece))
                pos += piece
        lits.append(x[pos:start + n])
        lit = np.concatenate(lits) if lits else np.zeros(0, np.uint8)
        rec = np.array(recs, dtype=np.uint32).reshape(-1, 2)
        replay(x, start, n, lit, rec, frame_start)
        out.append((lit, rec))
    return out


def replay(x, start, n, lit, rec, frame_start=0):
    """the block the records and literals stand for == x[start : start + n]"""
    got = bytearray(x[frame_start:start].tobytes())
    base, rank = len(got), 0
    for r, offml in rec.tolist():
        ml, off = offml & 255, offml >> 8
        got += lit[rank:r].tobytes()
        rank = r
        assert 3 <= ml and 1 <= off <= len(got), (ml, off, len(got))
        if off >= ml:
            got += got[len(got) - off:len(got) - off + ml]
        else:
            got += (bytes(got[len(got) - off:]) * (ml // off + 1))[:ml]
    got += lit[rank:].tobytes()
    assert len(got) - base == n and bytes(got[base:]) == x[start:start + n].tobytes(), "the parse does not reproduce the block"


def merged(seqs):
    """the sequences of one block as the encoder must write them: a sequence with no literals and the offset of the one in front of it is part of that one"""
    out = []
    for ll, ml, off in seqs:
        if out and ll == 0 and off == out[-1][2]:
            out[-1] = (out[-1][0], out[-1][1] + ml, off)
        else:
            out.append((ll, ml, off))
    return out
