"""The zstd encoder's entropy stage -- the literals kernel (gc_zstd_huf.hip), the four sequence kernels (gc_zstd_seq.hip), gc_fse.h and the launches they share with the
stream call (gc_api.hip zstd_entropy_part / zstd_join_and_emit) -- on EXACT parses, one named case per branch.  The test entry gc_test_zstd_encode_parsed (test builds only)
takes the literals and sequence records the match finder would have left, so a case decides what the kernels get; tests/zstd_parse.py composes the blocks and derives the
records; tests/zstd_inspect.py (a frame reader written from RFC 8878) says what the encoder wrote.  Every case asserts

    (a) the stream decodes to the input under the plain-C decoder of the oracle, the reference's decoder (where oracle/_ref is built) and this project's decoder,
    (b) the sequences the inspector reads, behind the repeat offsets, are exactly the parse that went in (chains merged),
    (c) the inspector shows the branch the case is named after,
    (d) on the device: the bytes are the emulator's.

A case is a frame of two blocks as a rule: 128 KiB of random bytes (stored raw; the history the matches copy from), then the block under test, short and last.

What the kernels decide differently from what one might expect, asserted as they decide it:
  * below 64 literals the section is raw whatever the bytes are (the reference does the same, zstd_compress_literals.c COMPRESS_LITERALS_SIZE_MIN): a repeated byte
    gives RLE literals from 64 up, so RLE headers come in 2 and 3 bytes only; the 1-byte RLE header cannot be reached.
  * `present > 1 << tl` in seq_build_table cannot hold (present <= min(nbSeq, maxSym + 1) and tl >= min(hibit(nbSeq) + 1, hibit(maxSym) + 2)), the predefined tables always
    hold every code a block can have (36 / 53 symbols; offset codes stop at 23 < 28 in an 8 MiB frame), and 26 222 sequences per block keep the 3-byte count out of reach.
  * a sequences section cannot outgrow a 4 KiB block of 3-byte matches: a sequence costs at most 17 offset bits and about 4 state bits in a frame of two blocks, under
    the 24 bits its match covers.  It does outgrow a block of a few matches (the section's fixed bytes): `overflow_tiny` is stored raw, `overflow_4k` stays compressed.

The geometric sweep of `test_huffman_trees` (60 000 literals; found with a trace of the limiter under the emulator that is not part of the tree):
    no limiter (depth <= 11)            ratio 1.2 at 16 and 32 symbols; 1.4 and 1.6 at 16
    clamp, debt repaid exactly          1.2 at 64; 1.4 and 1.6 at 32 (and the cases depth_12 and all_256_skewed)
    overshoot repair (debt < 0)         1.2 at 128, 256; 1.4 and 1.6 at 64, 128, 256; 1.8 and 2.0 at every size (and fibonacci_16); debts of -3 to -28, all brought back to 0
    give-up (debt != 0 -> raw)          none: no histogram tried here reaches it
(GEOMETRIC_PATH holds the same table; the test checks the part of it that shows from outside, depth <= 11 or not)."""
import heapq
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zstd_build as Z
import zstd_inspect as I
import zstd_parse as P
from zstd_build import LL, ML, OF

PRE, RLE, FSE = Z.MODE_PREDEFINED, Z.MODE_RLE, Z.MODE_FSE
BLOCK = P.BLOCK_MAX
R = np.random.default_rng(20260).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()      # block 0 of most cases
MAX_SEQ = BLOCK // 5 + 8                                                                 # GC_MAX_SEQ_PER_BLOCK


# ---------------------------------------------------------------------------------------------- the two backends
class Runner:
    def __init__(self, pkg, name, kw):
        self.name, self.pkg, self.kw = name, pkg, kw
        self.enc, self.dec = pkg.ZstdEncoder(level=3, **kw), pkg.ZstdDecoder(**kw)
        if name == "gpu":
            import torch
            self.torch = torch

    def encode(self, x, blocks):
        cap = self.enc.compress_bound(x.size)
        if self.name == "gpu":
            t = self.torch
            d_src, d_dst = t.from_numpy(np.array(x)).to("cuda:0"), t.full((cap,), 0xA5, dtype=t.uint8, device="cuda:0")
            t.cuda.synchronize()
            self.enc.code_parsed_device(d_src.data_ptr(), x.size, d_dst.data_ptr(), cap, blocks)
            return d_dst[:self.enc.finish()].cpu().numpy().tobytes()
        src, dst = np.ascontiguousarray(x), np.full(cap, 0xA5, np.uint8)
        self.enc.code_parsed_device(src.ctypes.data, x.size, dst.ctypes.data, cap, blocks)
        return dst[:self.enc.finish()].tobytes()

    def close(self):
        self.enc.close(); self.dec.close()


_EMU_BYTES = {}                                                    # case name -> the emulator's stream (assertion (d) compares the device's with it)


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def T(request, pkg):
    emu = Runner(pkg, "emu", dict(lib_path=request.getfixturevalue("emu_lib_path")))
    if request.param == "emu":
        yield emu
        emu.close()
        return
    gpu = Runner(pkg, "gpu", request.getfixturevalue("gpu_hooks_kw"))
    gpu.emu = emu
    yield gpu
    gpu.close(); emu.close()


def check(T, O, name, comp, cap=255, raw_blocks=()):
    """assertions (a), (b), (d) on a composed frame -> the inspector's frame"""
    x = comp.x()
    blocks = P.rows(x, comp.blocks, cap)
    s = T.encode(x, blocks)
    if T.name == "emu":
        _EMU_BYTES[name] = s
    else:
        if name not in _EMU_BYTES:
            _EMU_BYTES[name] = T.emu.encode(x, blocks)
        assert s == _EMU_BYTES[name], "%s: the device's bytes differ from the emulator's" % name                     # (d)
    a = np.frombuffer(s, dtype=np.uint8)
    assert np.array_equal(O.port_zstd_decompress(a, x.size), x), "%s: the oracle's decoder" % name                    # (a)
    if O.ref("zstd") is not None:
        assert np.array_equal(O.ref_zstd_decompress(a, x.size), x), "%s: the reference's decoder" % name
    assert np.array_equal(T.dec.code(a), x), "%s: this project's decoder" % name
    frames = I.inspect(s)
    assert len(frames) == 1 and frames[0].content == x.tobytes() and len(frames[0].blocks) == len(comp.blocks)
    for b, (blk, (_, n, seqs)) in enumerate(zip(frames[0].blocks, comp.blocks)):                                      # (b)
        assert len(blk.content) == n
        if b in raw_blocks or not seqs:
            assert blk.type == "raw" or (blk.type == "compressed" and blk.nseq == 0), "%s: block %d" % (name, b)
            continue
        assert blk.type == "compressed", "%s: block %d is stored %s" % (name, b, blk.type)
        got = [q[:3] for q in blk.resolved]
        want = P.merged(seqs)
        assert len(got) == len(want) == blk.nseq, "%s: block %d has %d sequences, the parse %d" % (name, b, len(got), len(want))
        if got != want:
            k = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError("%s: block %d sequence %d is %r, the parse says %r" % (name, b, k, got[k], want[k]))
    return frames[0]


def base():
    c = P.Composer()
    return c.lit(R).end_block(full=True)


def shuffled(counts, seed):
    """bytes with exactly this histogram ({symbol: count}), in an order that a seed fixes"""
    a = np.repeat(np.array(list(counts.keys()), dtype=np.uint8), list(counts.values()))
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def with_matches(c, lit):
    """the literals of a block cut in five around four fixed matches into block 0"""
    n = len(lit)
    cuts = [n // 4, n // 2, (3 * n) // 4, (7 * n) // 8]
    at = 0
    for cut, (ml, off) in zip(cuts, ((200, 70001), (37, 1234), (3, 99999), (600, 131072))):
        c.lit(lit[at:cut]).match(ml, off)
        at = cut
    return c.lit(lit[at:]).end_block()


def huffman_depths(counts):
    """the code lengths of an (unbounded) Huffman code for {symbol: count} -> {symbol: length}.  Among equal weights a leaf goes before a merged node and an older node
    before a newer one: of all optimal codes the one with the smallest depth"""
    heap = [(n, s, (s,)) for s, n in sorted(counts.items())]
    heapq.heapify(heap)
    depth, made = {s: 0 for s in counts}, 256
    while len(heap) > 1:
        n1, _, m1 = heapq.heappop(heap)
        n2, _, m2 = heapq.heappop(heap)
        for s in m1 + m2:
            depth[s] += 1
        heapq.heappush(heap, (n1 + n2, made, m1 + m2))
        made += 1
    return depth


# ---------------------------------------------------------------------------------------------- the entry refuses what the kernels were not sized for
def test_entry_refuses_bad_parses(T, pkg):
    x = np.frombuffer(R[:1000], dtype=np.uint8)
    lit = lambda n: x[:n]
    rec = lambda *rows: np.array(rows, dtype=np.uint32).reshape(-1, 2)
    bad = {"nLit above the block": (np.zeros(1001, np.uint8), rec()),
           "litRank above nLit": (lit(990), rec((991, (5 << 8) | 10))),
           "litRank decreasing": (lit(980), rec((500, (5 << 8) | 10), (499, (5 << 8) | 10))),
           "a match of 2": (lit(998), rec((500, (5 << 8) | 2))),
           "too few bytes": (lit(900), rec((500, (5 << 8) | 10))),
           "too many bytes": (lit(995), rec((500, (5 << 8) | 10))),
           "offset 0": (lit(990), rec((500, 10))),
           "offset in front of the frame": (lit(990), rec((500, (501 << 8) | 10))),
           "first sequence of a frame without literals": (lit(990), rec((0, (1 << 8) | 10))),
           "more records than the workspace holds": (lit(0), rec(*[(0, (1 << 8) | 3)] * (MAX_SEQ + 1)))}
    for what, blk in bad.items():
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
            T.encode(x, [blk])
    good = (lit(990), rec((500, (500 << 8) | 10)))                 # the largest offset that is inside is accepted
    assert len(I.content(T.encode(x, [good]))) == 1000
    shipped = getattr(pkg.load_library(), "gc_test_zstd_encode_parsed", None) if os.path.exists(pkg.LIB_PATH) else None
    assert shipped is None, "the shipped library exports the test entry"


# ---------------------------------------------------------------------------------------------- literals: type, header and streams at every size boundary
NLIT = (0, 1, 31, 32, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 16383, 16384)


def _literals(kind, n):
    if kind == "rle":
        return b"\x41" * n
    if kind == "flat":                                             # every value as often as every other: the largest count is ceil(n / 256) <= (n >> 7) + 4
        return shuffled({s: n // 256 + (1 if s < n % 256 else 0) for s in range(256) if n // 256 + (1 if s < n % 256 else 0)}, n)
    w = np.array([0.7 ** k for k in range(16)])                    # skewed: 16 symbols, the most frequent has about 30 %
    cnt = np.floor(w / w.sum() * n).astype(int)
    cnt[0] += n - cnt.sum()
    return shuffled({s: int(k) for s, k in enumerate(cnt) if k}, n)


@pytest.mark.parametrize("kind", ["rle", "flat", "skew"])
@pytest.mark.parametrize("n", NLIT)
def test_literals(T, O, kind, n):
    f = check(T, O, "literals_%s_%d" % (kind, n), with_matches(base(), _literals(kind, n)))
    li = f.blocks[1].lit
    assert li.regen == n and f.blocks[1].literals == _literals(kind, n)
    plain_header = 1 if n < 32 else (2 if n < 4096 else 3)
    if n < 64 or kind == "flat":
        assert (li.type, li.header_bytes) == ("raw", plain_header)
    elif kind == "rle":
        assert (li.type, li.header_bytes, li.comp) == ("rle", plain_header, 1)
    else:
        assert li.type == "compressed" and li.streams == (1 if n < 256 else 4)
        assert (li.header_bytes, li.size_format) == ((3, 0 if n < 256 else 1) if n < 1024 else ((4, 2) if n < 16384 else (5, 3)))
        assert max(li.tree.lengths) <= 11 and sum(1 for v in li.tree.lengths if v) == len(set(_literals(kind, n)))


def test_literals_whole_block(T, O):
    c = P.Composer().lit(_literals("skew", BLOCK)).end_block()
    f = check(T, O, "literals_whole_block", c)
    b = f.blocks[0]
    assert b.type == "compressed" and b.nseq == 0 and (b.lit.type, b.lit.regen, b.lit.header_bytes, b.lit.streams) == ("compressed", BLOCK, 5, 4)


# ---------------------------------------------------------------------------------------------- Huffman trees
def _scaled(weights, n):
    cnt = [max(1, int(round(w * n / sum(weights)))) for w in weights]
    return {s: k for s, k in enumerate(cnt)}


def _fib(k, scale):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return {s: v * scale for s, v in enumerate(f[:k])}


GEOMETRIC = [(r, k) for r in (1.2, 1.4, 1.6, 1.8, 2.0) for k in (16, 32, 64, 128, 256)]
# what the limiter did in each row of the sweep (see the docstring of this file): "free" (an unbounded code has at most 11 bits: no limiter), "clamp" (clamped, and lengthening
# rare symbols repaid the debt exactly), "overshoot" (the repayment went below zero and frequent 11-bit codes were shortened).  From outside only "free" can be told apart.
GEOMETRIC_PATH = {(r, k): ("free" if (r, k) in ((1.2, 16), (1.2, 32), (1.4, 16), (1.6, 16)) else "clamp" if (r, k) in ((1.2, 64), (1.4, 32), (1.6, 32)) else "overshoot")
                  for r, k in GEOMETRIC}
TREES = {
    "fibonacci_16": _fib(16, 23),                                  # depth 15
    "depth_11": _fib(12, 159),
    "depth_12": _fib(13, 98),
    "two_symbols": {0: 45000, 1: 15000},
    "symbols_0_255": {0: 45000, 255: 15000},
    "top_symbol_128": dict([(s, 100) for s in range(128)] + [(128, 12800)]),       # 128 weights of one value: no FSE form, the direct one just fits
    "top_symbol_129": dict([(s, 100) for s in range(1, 129)] + [(129, 12800)]),    # 129 weights: only the FSE form
    "no_describable_tree": dict([(s, 10) for s in range(254)] + [(254, 25)]),      # 254 weights of one value and too many for the direct form
    "no_describable_tree_192": dict([(s, 10) for s in range(192)] + [(192, 1280)]), # 192 weights of one value (8 bits; symbol 192 has 2): a code that would save a quarter
    "all_256_skewed": _scaled([1.02 ** -k for k in range(256)], 60000),
    "gain_below_min": dict([(s, 16) for s in range(255)] + [(255, 40)]),           # 4120 literals at 7.99 bits each
}
TREES.update({"geometric_%.1f_%d" % (r, k): _scaled([r ** -i for i in range(k)], 60000) for r, k in GEOMETRIC})


def _tree_checks(li, counts):
    """a complete prefix code of at most 11 bits in which every present symbol has a length and no absent one"""
    t = li.tree
    assert max(t.lengths) <= 11 and sum(2 ** (11 - n) for n in t.lengths if n) == 2 ** 11
    assert [s for s in range(256) if t.lengths[s]] == sorted(counts)


@pytest.mark.parametrize("name", sorted(TREES))
def test_huffman_trees(T, O, name):
    counts = TREES[name]
    lit = shuffled(counts, 7)
    f = check(T, O, "tree_" + name, with_matches(base(), lit))
    li = f.blocks[1].lit
    depth = huffman_depths(counts)
    deepest, cost = max(depth.values()), sum(counts[s] * depth[s] for s in counts)
    if li.type == "compressed":
        _tree_checks(li, counts)
        got_cost = sum(counts[s] * li.tree.lengths[s] for s in counts)
        assert got_cost >= cost and (deepest > 11 or got_cost == cost), "a code of %d bits where the optimum is %d" % (got_cost, cost)
    if name == "fibonacci_16":
        assert deepest == 15 and li.type == "compressed" and max(li.tree.lengths) == 11
    elif name == "depth_11":
        assert deepest == 11 and li.type == "compressed" and max(li.tree.lengths) == 11 and [li.tree.lengths[s] for s in sorted(counts)] == [depth[s] for s in sorted(counts)]
    elif name == "depth_12":
        assert deepest == 12 and li.type == "compressed" and max(li.tree.lengths) == 11
    elif name == "two_symbols":
        assert li.type == "compressed" and (li.tree.kind, li.tree.weights) == ("direct", [1])
    elif name == "symbols_0_255":
        assert li.type == "compressed" and li.tree.kind == "fse" and len(li.tree.weights) == 255
    elif name == "top_symbol_128":
        assert li.type == "compressed" and (li.tree.kind, li.tree.weights) == ("direct", [1] * 128)
    elif name == "top_symbol_129":
        assert li.type == "compressed" and (li.tree.kind, li.tree.weights) == ("fse", [0] + [1] * 128)
    elif name == "no_describable_tree":
        # the input's condition: the (unbounded, unique up to ties) code gives symbols 0..253 one length, and the section is not raw for another reason
        assert len({depth[s] for s in range(254)}) == 1 and max(counts.values()) > (len(lit) >> 7) + 4
        assert li.type == "raw"
    elif name == "no_describable_tree_192":
        # ... and here the streams alone would leave far more than minGain: raw can only be the missing description
        assert len({depth[s] for s in range(192)}) == 1 and max(counts.values()) > (len(lit) >> 7) + 4 and cost // 8 + 64 < len(lit) - (len(lit) >> 6) - 2
        assert li.type == "raw"
    elif name == "all_256_skewed":
        assert li.type == "compressed" and li.tree.kind == "fse" and len(li.tree.weights) == 255
    elif name == "gain_below_min":
        # the input's condition: past the "flat histogram" test, a code that needs no limiter and has an FSE description, whose streams alone leave less than minGain
        assert max(counts.values()) > (len(lit) >> 7) + 4 and deepest <= 11 and len(set(depth.values())) > 1
        assert cost // 8 + (len(lit) >> 6) + 2 >= len(lit) and li.type == "raw"
    else:
        r, k = [(r, k) for r, k in GEOMETRIC if name == "geometric_%.1f_%d" % (r, k)][0]
        assert li.type in ("compressed", "raw")                    # complete and at most 11 bits (above), or stored raw
        assert (deepest <= 11) == (GEOMETRIC_PATH[(r, k)] == "free"), "the table of the sweep is stale: depth %d" % deepest
        assert li.type == "compressed"                             # ... and no row of the sweep gives up (the docstring's table)


# ---------------------------------------------------------------------------------------------- sequences: counts
def _mixed(c, n, seed, ll_hi=6, ml_hi=12):
    """n sequences of a mixed kind behind block 0: short literal runs (some empty), short matches, offsets over the whole history"""
    rng = np.random.default_rng(seed)
    lls, mls = rng.integers(0, ll_hi + 1, n), rng.integers(3, ml_hi + 1, n)
    lits = rng.integers(0, 256, int(lls.sum()) + 3, dtype=np.uint8).tobytes()
    at = 0
    for ll, ml in zip(lls.tolist(), mls.tolist()):
        c.lit(lits[at:at + ll])
        at += ll
        while True:
            off = int(rng.integers(1, len(c.out) + 1)) if rng.integers(0, 8) else int(rng.integers(1, 9))
            if ll or not c.seqs or off != c.seqs[-1][2]:           # (no literals and the offset in front of it: that would be one sequence, and the count is the case)
                break
        c.match(ml, off)
    return c.lit(lits[at:at + 3]).end_block()


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193])
def test_sequence_counts(T, O, n):
    f = check(T, O, "nseq_%d" % n, _mixed(base(), n, n, ml_hi=12 if n >= 64 else 40))      # (a block of a few short matches would not beat its raw form)
    b = f.blocks[1]
    assert b.nseq == n and b.nseq_bytes == (1 if n < 128 else 2)
    if n == 1:
        assert b.modes == [RLE, RLE, RLE] and b.logs == [0, 0, 0]
    if n == 2:
        assert b.modes == [PRE, PRE, PRE]
    if n >= 1023:
        assert b.modes == [FSE, FSE, FSE]
    if n == 8193:
        assert b.logs == [9, 8, 9]                                 # tl clamped at the top


def test_most_sequences_a_block_holds(T, O):
    """131070 bytes of 5-byte matches without literals: 26 214 sequences (the workspace holds 26 222)"""
    c = base()
    rng = np.random.default_rng(5)
    offs = rng.integers(5, 2000, BLOCK // 5)
    offs[1:][offs[1:] == offs[:-1]] += 1                           # (a neighbour with the same offset would merge)
    assert not np.any(offs[1:] == offs[:-1])
    for off in offs.tolist():
        c.match(5, off)
    f = check(T, O, "nseq_most", c.lit(b"zz").end_block(full=True))
    assert f.blocks[1].nseq == BLOCK // 5 == 26214 and f.blocks[1].nseq_bytes == 2 and f.blocks[1].modes[LL] == RLE and f.blocks[1].modes[ML] == RLE


# ---------------------------------------------------------------------------------------------- sequences: table modes
def _seqs(c, rows, seed=3):
    lits = np.random.default_rng(seed).integers(0, 256, sum(r[0] for r in rows) + 2, dtype=np.uint8).tobytes()
    at = 0
    for ll, ml, off in rows:
        c.lit(lits[at:at + ll]).match(ml, off)
        at += ll
    return c.lit(lits[at:at + 2]).end_block()


def _varied(n, seed, ll=None, ml=None, of_code=None):
    """n sequences whose literal length / match length / offset code is fixed where given and varied where not; no offset repeats one of the two in front"""
    rng = np.random.default_rng(seed)
    rows, prev = [], [0, 0]
    for i in range(n):
        while True:
            off = int(rng.integers((1 << of_code) - 3, (2 << of_code) - 3)) if of_code is not None else int(rng.integers(8, 100000))
            if off not in prev and off + 1 != prev[-1]:
                break
        prev = [prev[-1], off]
        rows.append((int(rng.integers(1, 12)) if ll is None else ll, int(rng.integers(4, 30)) if ml is None else ml, off))
    return rows


@pytest.mark.parametrize("which", ["LL", "OF", "ML", "all"])
def test_one_code_only_is_an_rle_table(T, O, which):
    rows = _varied(40, 11, ll=2 if which in ("LL", "all") else None, ml=7 if which in ("ML", "all") else None, of_code=10 if which in ("OF", "all") else None)
    f = check(T, O, "rle_table_" + which, _seqs(base(), rows))
    b = f.blocks[1]
    want = {"LL": [True, False, False], "OF": [False, True, False], "ML": [False, False, True], "all": [True, True, True]}[which]
    assert [m == RLE for m in b.modes] == want and [s is not None for s in b.rle_syms] == want
    if which == "all":
        assert b.rle_syms == [2, 10, 4] and b.seq_section_bytes == 1 + 1 + 3 + (40 * 10 + 1 + 7) // 8      # no state bits at all: ten offset bits per sequence and the end mark


def test_few_sequences_take_the_predefined_tables(T, O):
    f = check(T, O, "predefined_tables", _seqs(base(), _varied(6, 12)))
    assert f.blocks[1].modes == [PRE, PRE, PRE] and f.blocks[1].logs == [6, 5, 6]


@pytest.mark.parametrize("which", ["LL", "ML", "OF"])
def test_codes_behind_the_predefined_tables_counts(T, O, which):
    """codes whose cells in the predefined tables are "less than one" (literal lengths from 8192, matches from 1027), and the largest offset code two blocks allow: whatever
    mode the cost comparison takes, the codes are there and the stream is legal (the inspector and three decoders read it)"""
    c = base()
    if which == "LL":
        rows = [(8192, 200, 5000), (3, 9, 77), (16384 + 5, 300, 131072), (1, 5, 9)]
    elif which == "ML":
        rows = [(2, 1027, 131072), (3, 9, 77), (4, 5000, 70000), (1, 40000, 131070)]
    else:
        c = P.Composer().lit(R).end_block(full=True).lit(R[:1000])
        rows = [(0, 50, BLOCK + 1000 - 3), (4, 9, 77), (2, 60, BLOCK + 500), (1, 5, 9)]
    f = check(T, O, "top_code_" + which, _seqs(c, rows))
    b = f.blocks[1]
    codes = [q[{"LL": 0, "OF": 1, "ML": 2}[which]] for q in b.codes]
    assert max(codes) == {"LL": 33, "ML": 51, "OF": 17}[which]
    for w in (LL, OF, ML):
        assert b.modes[w] in (PRE, RLE, FSE) and (b.modes[w] != FSE or sum(abs(v) for v in b.norms[w]) == 1 << b.logs[w])


@pytest.mark.parametrize("n", [32, 33])
def test_as_many_match_length_codes_as_sequences(T, O, n):
    """every sequence has a match-length code of its own: the table, whichever mode it has, holds them all"""
    rows = [(1 + i % 3, Z.ML_BASE[i], off) for i, (_, _, off) in enumerate(_varied(n, 13))]
    f = check(T, O, "ml_codes_%d" % n, _seqs(base(), rows))
    b = f.blocks[1]
    assert sorted(q[2] for q in b.codes) == list(range(n)) and b.modes[ML] in (PRE, FSE)
    assert sum(1 for v in b.norms[ML] if v) >= n and (1 << b.logs[ML]) >= n


def test_every_cell_demoted(T, O):
    """128 sequences, match-length codes 0..15 eight times each: log 5, every normalised count 2, every one demoted to 1 -- the largest as well, which then takes the 16 freed"""
    mls = np.repeat(np.arange(3, 19), 8)
    np.random.default_rng(14).shuffle(mls)
    rows = [(2, int(ml), off) for ml, (_, _, off) in zip(mls.tolist(), _varied(128, 14, of_code=11))]
    f = check(T, O, "every_cell_demoted", _seqs(base(), rows))
    b = f.blocks[1]
    assert (b.modes[ML], b.logs[ML], b.norms[ML]) == (FSE, 5, [17] + [1] * 15)
    assert b.modes[LL] == RLE and b.modes[OF] == RLE


# ---------------------------------------------------------------------------------------------- sequences: extreme values
def test_longest_literal_run(T, O):
    n = 65536 + 7
    f = check(T, O, "ll_65543", _seqs(base(), [(n, 3000, 131072), (2, 9, 7)]))
    assert f.blocks[1].resolved[0][:3] == (n, 3000, 131072) and f.blocks[1].codes[0][0] == 35


def test_one_match_fills_the_block(T, O):
    """5 literals and one match of 131 067 bytes at offset 1: 514 records of 255 and one of 252, merged; match-length code 52"""
    c = base().lit(b"abcde").match(BLOCK - 5, 1).end_block(full=True)
    f = check(T, O, "ml_131067", c)
    assert f.blocks[1].resolved == [(5, BLOCK - 5, 1, "new")] and f.blocks[1].codes[0][2] == 52


def test_shortest_matches(T, O):
    f = check(T, O, "ml_3_and_4", _seqs(base(), [(1, 3, 500), (0, 4, 900), (2, 3, 7), (0, 3, 100000), (1, 4, 3), (5, 40, 60000)]))
    assert [q[1] for q in f.blocks[1].resolved] == [3, 4, 3, 3, 4, 40]


@pytest.mark.parametrize("k", [3, 8, 16, 17])
def test_offsets_at_a_power_of_two(T, O, k):
    """offset value 2^k exactly (code k, extra bits 0) and 2^k - 1 (code k - 1, extra bits all 1)"""
    f = check(T, O, "offset_2^%d" % k, _seqs(base(), [(3, 12, (1 << k) - 3), (2, 12, (1 << k) - 4), (4, 12, 50), (1, 12, (1 << k) - 3)]))
    b = f.blocks[1]
    assert [q[2] for q in b.seqs][:2] == [1 << k, (1 << k) - 1] and [q[1] for q in b.codes][:2] == [k, k - 1]


# ---------------------------------------------------------------------------------------------- repeat offsets
A_, B_ = 3000, 777


def test_every_repeat_form(T, O):
    rows = [(5, 10, A_), (3, 10, A_), (2, 10, B_), (1, 10, A_), (0, 10, B_), (0, 10, B_ - 1), (0, 10, B_ - 1), (4, 10, 9)]
    f = check(T, O, "repeat_forms", _seqs(base(), rows))
    b = f.blocks[1]
    assert [q[3] for q in b.resolved] == ["new", "rep1", "new", "rep2", "rep2", "rep1-1", "new"]
    assert b.resolved[5][:3] == (0, 20, B_ - 1)                    # ll == 0 with the offset in front of it: merged, there is no code for it
    assert [q[2] for q in b.seqs][:6] == [A_ + 3, 1, B_ + 3, 2, 1, 3]


@pytest.mark.parametrize("off,form", [(1, "rep1"), (4, "rep2")])
def test_first_sequence_of_a_frame(T, O, off, form):
    """the history a frame starts with: {1, 4, 8}"""
    c = P.Composer().lit(b"abcdefgh").match(20, off).lit(b"xy").match(9, 3).lit(b"!").end_block()
    f = check(T, O, "frame_start_off_%d" % off, c)
    assert f.blocks[0].resolved[0] == (8, 20, off, form) and f.blocks[0].seqs[0][2] == (1 if off == 1 else 2)


@pytest.mark.parametrize("ll", [3, 0])
@pytest.mark.parametrize("off", [1, 4])
def test_first_sequence_of_a_later_block(T, O, off, ll):
    """the same parses as a frame's second block: the history is what block 0 left, which this block's coder does not know -- no repeat code"""
    c = base().lit(b"abc"[:ll]).match(20, off).lit(b"xy").match(9, 3).lit(b"!").end_block()
    f = check(T, O, "later_block_off_%d_ll_%d" % (off, ll), c)
    assert f.blocks[1].resolved[0] == (ll, 20, off, "new")


def test_repeat_offset_1_and_no_literals(T, O):
    """rep1 == 1 and ll == 0: "rep1 - 1" would be offset 0"""
    f = check(T, O, "rep1_is_1", _seqs(base(), [(4, 10, 1), (0, 10, 7), (0, 10, 6), (3, 10, 1), (0, 12, 2)]))
    assert [q[3] for q in f.blocks[1].resolved] == ["new", "new", "rep1-1", "new", "new"]


# ---------------------------------------------------------------------------------------------- chains of capped records
def test_chain_lengths(T, O):
    rows = [(2, 255, 131072), (3, 256, 70000), (1, 510, 131072), (2, 511, 5), (0, 255, 9), (1, 9, 40)]
    c = _seqs(base(), rows)
    assert [len(P.split(r[1], 255)) for r in rows] == [1, 2, 2, 3, 1, 1]
    f = check(T, O, "chain_lengths", c)
    assert [q[1] for q in f.blocks[1].resolved] == [255, 256, 510, 511, 255, 9]


@pytest.mark.parametrize("lead,chain", [(10, 245), (10, 246), (10, 247), (250, 12), (255, 2), (256, 2), (0, 600), (1100, 300)])
def test_chain_across_rounds_and_ring(T, O, lead, chain):
    """`lead` one-record sequences, then one match of `chain` records (cap 6): chains that end at, or run over, the 256 records the codes kernel takes per round, a chain of
    600 records, and one behind 1100 sequences, where the ring of 1024 merged sequences has wrapped"""
    c = base()
    for i in range(lead):
        c.lit(bytes([i & 255])).match(4, 2000 + 2 * i)
    c.lit(b"q").match(6 * chain, 131072).lit(b"rs").match(5, 3)
    c.end_block()
    blocks = P.rows(c.x(), c.blocks, cap=6)
    assert blocks[1][1].shape[0] == lead + chain + 1
    f = check(T, O, "chain_%d_%d" % (lead, chain), c, cap=6)
    assert f.blocks[1].nseq == lead + 2 and f.blocks[1].resolved[lead][:3] == (1, 6 * chain, 131072)


def test_two_chains_back_to_back(T, O):
    f = check(T, O, "chains_back_to_back", _seqs(base(), [(3, 700, 131072), (0, 700, 70000), (0, 300, 131072), (2, 8, 5)]))
    assert [q[:3] for q in f.blocks[1].resolved] == [(3, 700, 131072), (0, 700, 70000), (0, 300, 131072), (2, 8, 5)]


# ---------------------------------------------------------------------------------------------- state chains
def _four_codes(rare_u=None):
    """8292 sequences, every table's codes drawn from four equiprobable ones (literal lengths 0..3, match lengths 3..6, offset codes 9..12) and no repeat offset: no count-1
    symbol, so no two state walks are sure to meet.  (Drawn, not dealt: with exactly 2073 of each the normalised counts are 128 each, every step drops exactly two bits
    of the state, and all walks have met after a few steps -- one round.)  rare_u: the sequence that the walk reaches as its element rare_u (the walk goes backwards) gets a literal length of its own."""
    n = 8292
    rng = np.random.default_rng(99)
    cols = [rng.integers(0, 4, n) for _ in range(3)]
    rows, prev = [], [0, 0]
    for i in range(n):
        c = 9 + int(cols[2][i])
        while True:
            off = int(rng.integers((1 << c) - 3, (2 << c) - 3))
            if off not in prev and off + 1 != prev[-1]:
                break
        prev = [prev[-1], off]
        ll = int(cols[0][i])
        if rare_u is not None and i == n - 1 - rare_u:
            ll = 9
        rows.append((ll, 3 + int(cols[1][i]), off))
    return _seqs(base(), rows)


def test_state_chains_with_no_meeting_point(T, O, capfd, monkeypatch):
    if T.name == "emu":
        monkeypatch.setenv("GC_TRACE_CHAIN", "1")
        capfd.readouterr()
    f = check(T, O, "four_codes", _four_codes())
    b = f.blocks[1]
    assert b.nseq == 8292 and b.modes == [FSE, FSE, FSE] and b.logs == [9, 8, 9]
    assert all(len([v for v in b.norms[w] if v]) == 4 and min(v for v in b.norms[w] if v) > 1 for w in (LL, OF, ML))
    if T.name == "emu":
        rounds = [int(m) for m in re.findall(r"chain table=\d+ tile=\d+ len=\d+ L=\d+ rounds=(\d+)", capfd.readouterr().err)]
        assert len(rounds) == 9 and max(rounds) >= 32, rounds     # three tables, tiles of 4096 + 4096 + 100


@pytest.mark.parametrize("back", [256, 257, 320])
def test_state_chains_one_meeting_point(T, O, back):
    """one count-1 symbol 4 segments (256 sequences) in front of a segment's start -- the last place a lane looks for one --, one further, and 5 segments in front"""
    f = check(T, O, "four_codes_rare_%d" % back, _four_codes(rare_u=10 * 64 - back))
    b = f.blocks[1]
    assert b.modes[LL] == FSE and sorted(abs(v) for v in b.norms[LL] if v)[0] == 1 and b.codes[8292 - 1 - (640 - back)][0] == 9


def test_every_symbol_once(T, O):
    """a table in which every present symbol has count 1 (every state walk meets at every step)"""
    rows = [(i, Z.ML_BASE[20 + i], 100 * (1 << i)) for i in range(10)]
    f = check(T, O, "every_symbol_once", _seqs(base(), rows))
    b = f.blocks[1]
    assert all(len(set(q[w] for q in b.codes)) == 10 for w in range(3))
    for w in (LL, OF, ML):
        assert b.modes[w] in (PRE, FSE)


# ---------------------------------------------------------------------------------------------- a sequences section that outgrows its block
def _far_matches(c, nbytes, seed):
    rng = np.random.default_rng(seed)
    prev = 0
    for _ in range(nbytes // 3):
        while True:
            off = int(rng.integers(1 << 16, BLOCK + c.here()))
            if off != prev:
                break
        prev = off
        c.match(3, off)
    return c


def _middle_block(c):
    """a full block that compresses well, between block 0 and the block under test"""
    return c.lit(b"middle").match(BLOCK - 6 - 1000, BLOCK).lit(R[:1000][::-1]).end_block(full=True)


def test_overflow_tiny(T, O):
    """three 3-byte matches at far offsets: 9 bytes of content; the section has 4 bytes in front of its bitstream (count, modes, the RLE symbols of two tables) and at
    least 3 x 16 offset bits, 5 bits of the offsets' first state and the end mark in it, 11 bytes -> the block is stored raw; the block in front of it is compressed as ever"""
    c = _far_matches(_middle_block(base()), 9, 21).end_block()
    f = check(T, O, "overflow_tiny", c, raw_blocks=(2,))
    assert [b.type for b in f.blocks] == ["raw", "compressed", "raw"] and f.blocks[2].content == c.x()[2 * BLOCK:].tobytes()
    assert f.blocks[1].resolved == [(6, BLOCK - 1006, BLOCK, "new")]


def test_overflow_4k(T, O):
    """4 KiB of 3-byte matches at far offsets (1365 sequences): about 18 bits each, a section of three quarters of the block -- it stays compressed"""
    c = _far_matches(_middle_block(base()), 4096, 22).lit(b"!").end_block()
    f = check(T, O, "overflow_4k", c)
    b = f.blocks[2]
    assert b.type == "compressed" and b.nseq == 1365 and b.modes[LL] == RLE and b.modes[ML] == RLE and b.seq_section_bytes < 4096
    assert f.blocks[1].resolved == [(6, BLOCK - 1006, BLOCK, "new")]


# ---------------------------------------------------------------------------------------------- the inspector itself (CPU only)
def _handmade():
    import hashlib
    z = np.load(os.path.join(HERE, "golden", "zstd_handmade.npz"))
    names = z["names"].tobytes().decode().split("\0")
    at = np.concatenate([[0], np.cumsum(z["stream_sizes"])])
    return {nm: (z["streams"][at[i]:at[i + 1]].tobytes(), bool(z["flags"][i][0]), z["shas"][i].tobytes(), int(z["flags"][i][5])) for i, nm in enumerate(names)}, hashlib


def test_inspector_reads_the_handmade_frames(O):
    """every accepted stream of tests/golden/zstd_handmade.npz: the content the reference made of it (the fixture's SHA-256) and the oracle's decoder makes of it"""
    cases, hashlib = _handmade()
    n = ported = 0
    for name, (stream, accepted, sha, size) in cases.items():
        if not accepted:
            continue
        got = I.content(stream)
        assert len(got) == size and hashlib.sha256(got).digest() == sha, name
        if size and not name.startswith("did_") and size <= (1 << 20):      # (the oracle's decoder takes no dictionary-id field, and no frame beyond its buffer)
            assert O.port_zstd_decompress(np.frombuffer(stream, dtype=np.uint8), size).tobytes() == got, name
            ported += 1
        n += 1
    assert n > 100 and ported > 90


def test_inspector_reports_what_the_builder_wrote():
    cases, _ = _handmade()
    combos = [[a, b, c] for a in (PRE, RLE, FSE) for b in (PRE, RLE, FSE) for c in (PRE, RLE, FSE)]
    blocks = [b for f in I.inspect(cases["modes_27_combinations"][0]) for b in f.blocks if b.type == "compressed" and b.nseq]
    assert [b.modes for b in blocks[-27:]] == combos
    # a frame of the builder, field by field
    f = Z.Frame()
    f.raw(bytes(range(100)))
    h = Z.Huffman([4, 3, 2, 1, 1])
    lit = bytes([0, 1, 0, 2, 0, 3, 4, 0, 1, 0] * 30)
    f.compressed(Z.lit_huf(h, lit, 0), lit, [(4, 5, 40), (0, 7, 33), (3, 300, 50), (2, 4, 35)], modes=(PRE, RLE, FSE), huf=h,
                 specs=(None, 5, (Z.dist(53, {1: 8, 2: 8, 4: 8, 44: 8}), 5)))
    f.compressed(Z.lit_rle(9, 40), b"\x09" * 40, [(1, 3, 1)], modes=(RLE, RLE, RLE), specs=(1, 0, 0), nseq_form=2, last=True)
    assert f.sound
    frames = I.inspect(f.bytes(fcs=len(f.out), single=True))
    assert len(frames) == 1 and frames[0].content == bytes(f.out)
    _, b0, b1 = frames[0].blocks
    assert (b0.lit.type, b0.lit.size_format, b0.lit.streams, b0.lit.regen, b0.lit.tree.kind, b0.lit.tree.weights) == ("compressed", 0, 1, 300, "direct", [4, 3, 2, 1])
    assert b0.lit.tree.lengths[:6] == [1, 2, 3, 4, 4, 0] and b0.literals == lit
    assert (b0.nseq, b0.nseq_bytes, b0.modes, b0.logs) == (4, 1, [PRE, RLE, FSE], [6, 0, 5]) and b0.rle_syms == [None, 5, None]
    assert b0.norms[ML][:5] == [0, 8, 8, 0, 8] and b0.norms[ML][44] == 8 and b0.norms[OF] is None
    assert b0.seqs == [(4, 5, 40), (0, 7, 33), (3, 300, 50), (2, 4, 35)]
    assert b0.resolved == [(4, 5, 37, "new"), (0, 7, 30, "new"), (3, 300, 47, "new"), (2, 4, 32, "new")]
    assert (b1.lit.type, b1.lit.regen, b1.lit.header_bytes, b1.nseq, b1.nseq_bytes, b1.modes) == ("rle", 40, 2, 1, 2, [RLE, RLE, RLE])
    assert b1.resolved == [(1, 3, 32, "rep1")]
    # the 3-byte form of the sequence count
    assert Z.nseq_bytes(0x7F00 + 5, 3) == b"\xff\x05\x00"


def test_inspector_reads_the_reference_encoders_stream(O):
    comp = open(os.path.join(HERE, "golden", "test.txt.zstd"), "rb").read()
    frames = I.inspect(comp)
    got = b"".join(f.content for f in frames)
    assert got == O.port_zstd_decompress(np.frombuffer(comp, dtype=np.uint8), 2_000_000).tobytes() and len(got) == 1_000_000
    assert any(b.type == "compressed" and b.nseq for f in frames for b in f.blocks) and any(b.type == "rle" for f in frames for b in f.blocks)
