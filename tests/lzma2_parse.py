"""Exact parses for the LZMA2 encoder's back end (tests/test_lzma2_stages.py): the input is COMPOSED from literals and matches, which gives both the bytes and the parse;
`rows` turns the parse into the records the match finder would have left (gc_common.h GcSeqRaw: literals of the block in front of the match, offset << 8 | length, length
1..255 -- a longer match is a chain of records of one offset with no literals between them); `expected` says which match-type symbols the encoder has to make of them.

`expected` is plain sequential Python, derived from the LZMA format and from what gc_lzma2.h says about the item list -- not from the kernels' scans:
  * neighbouring records of one offset with no literals between them are ONE match;
  * a match is cut at every 4 KiB boundary of the block; a piece of ONE byte that a boundary leaves at either end of a match is given up (those bytes are literals);
  * a piece is cut every 273 bytes, the longest LZMA match, but never so that one byte remains: 274 = 272 + 2;
  * the decoder keeps four repeat distances, most recently used first, all 1 behind a state reset, i.e. at every model-segment start.  A piece whose distance is in the
    list is coded as that repeat -- the first entry that holds it; only entries 0 and 1 without rep4 -- and moves to the front; any other distance is a match and pushes the last
    entry out;
  * a one-byte piece is a short rep if its distance is the list's front (the list stays as it is), and a literal otherwise."""
import numpy as np

BLOCK_MAX = 1 << 17
RC = 1 << 12
MATCH, SHORTREP, REPS = "match", "short rep", ("rep0", "rep1", "rep2", "rep3")


class Composer:
    """The input, block by block.  lit(bytes) / match(ml, dist) append to the open block; end_block() closes it.  `blocks`: per block (start, length,
    [(ll, ml, dist)]) -- the literals behind the last match are the rest of the block."""
    def __init__(self):
        self.out, self.blocks, self.start, self.seqs, self.ll = bytearray(), [], 0, [], 0

    def lit(self, data):
        data = bytes(data)
        self.out += data
        self.ll += len(data)
        return self

    def match(self, ml, dist):
        n = len(self.out)
        assert ml >= 1 and 1 <= dist <= n, (ml, dist, n)
        if dist >= ml:
            self.out += self.out[n - dist:n - dist + ml]
        else:
            self.out += (bytes(self.out[n - dist:]) * (ml // dist + 1))[:ml]
        self.seqs.append((self.ll, ml, dist))
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


def rows(x, blocks, cap=255):
    """blocks as Composer.blocks -> [(number of literals, records (k, 2) uint32)] for Flzma2Encoder.code_parsed_device; the records are replayed against x"""
    out = []
    for start, n, seqs in blocks:
        recs, rank = [], 0
        for ll, ml, dist in seqs:
            rank += ll
            while ml > 0:
                take = min(ml, cap)
                recs.append((rank, (dist << 8) | take))
                ml -= take
        rec = np.array(recs, dtype=np.uint32).reshape(-1, 2)
        nlit = n - sum(ml for _, ml, _ in seqs)
        replay(x, start, n, rec)
        out.append((nlit, rec))
    return out


def replay(x, start, n, rec):
    """the block the records stand for == x[start : start + n] (the literals are taken from x itself: LZMA's records carry none)"""
    got = bytearray(x[:start].tobytes())
    rank = 0
    for r, offml in rec.tolist():
        ml, dist = offml & 255, offml >> 8
        got += x[len(got):len(got) + r - rank].tobytes()
        rank = r
        assert 1 <= ml and 1 <= dist <= len(got), (ml, dist, len(got))
        for _ in range(ml):
            got.append(got[len(got) - dist])
    got += x[len(got):start + n].tobytes()
    assert len(got) == start + n and bytes(got[start:]) == x[start:start + n].tobytes(), "the parse does not reproduce the block"


def pieces(pos, ml):
    """a match of ml bytes at block position pos as the encoder codes it: [(position, length)]"""
    start, end = pos, pos + ml
    if ml > 1 and (start + 1) % RC == 0:                             # one byte in front of a boundary, the rest behind it
        start += 1
    if end - start > 1 and (end - 1) % RC == 0:                      # one byte behind a boundary, the rest in front of it
        end -= 1
    out = []
    while start < end:
        stop = min(end, (start // RC + 1) * RC)
        while start < stop:
            take = min(stop - start, 273)
            if stop - start - take == 1:
                take -= 1
            out.append((start, take))
            start += take
    return out


def expected(blocks, seg_log=17, rep4=True, leaders=None, stored=()):
    """the match-type symbols of the stream, [(position in the input, kind, length, distance)].  seg_log: the level's model segment (14 at level 1, 15 at level 3, 17 at
    5 and 7); leaders: with 128 KiB segments, the blocks that start a model segment (None: every block); stored: the model segments (numbered from the input's
    start in units of 2^seg_log) that the encoder stores -- they have no symbols."""
    out, reps, seg_now = [], [1, 1, 1, 1], None
    for b, (start, n, seqs) in enumerate(blocks):
        if seg_log == 17 and (leaders is None or b in leaders):
            reps = [1, 1, 1, 1]
        matches, pos = [], 0
        for ll, ml, dist in seqs:
            pos += ll
            if matches and ll == 0 and matches[-1][2] == dist:
                matches[-1][1] += ml
            else:
                matches.append([pos, ml, dist])
            pos += ml
        for mpos, ml, dist in matches:
            for p, take in pieces(mpos, ml):
                seg = (start + p) >> seg_log
                if seg != seg_now:                                   # (segments smaller than a block: every one of them starts with a reset)
                    seg_now = seg
                    if seg_log < 17:
                        reps = [1, 1, 1, 1]
                if seg in stored:
                    continue
                if take == 1:
                    if dist == reps[0]:
                        out.append((start + p, SHORTREP, 1, dist))
                    continue
                look = reps if rep4 else reps[:2]
                if dist in look:
                    k = look.index(dist)
                    out.append((start + p, REPS[k], take, dist))
                    del reps[k]
                else:
                    out.append((start + p, MATCH, take, dist))
                    reps.pop()
                reps.insert(0, dist)
    return out
