"""The sequence stage of the zstd encoder at the edges of its rounds.  gc_zstd_seq.hip takes R = 4 raw records per thread and round in the codes kernel (N = 256 * R = 1024
per workgroup; merged sequences wait in a ring of G = 4 * N) and R sequences per thread and round in the pack kernel, where a wave takes R slabs of 64 neighbouring
sequences.  The cases put what the kernels treat specially -- heads, chains of capped records, runs of equal offsets, the repeat-offset forms that depend on a literal
length of 0, fat sequences, the bits carried from one round's tile into the next -- in front of, on and behind the edges of a thread's records, a wave's, a round's and
the ring's.  Exact parses go in through the parsed test entry (tests/zstd_parse.py composes them, tests/zstd_inspect.py reads what came out); frames are two blocks,
128 KiB of random bytes and then the block under test.  Every case asserts

    (a) the stream decodes under the oracle's plain-C decoder, the reference's decoder (where oracle/_ref is built) and this project's decoder,
    (b) the inspector reads exactly the parse that went in (chains merged),
    (c) the bytes are those of the emulator build of the commit in front of the change that introduced these rounds (tests/golden/seq_rounds/streams.npz, written by
        tools/record_seq_rounds.py: per case the SHA-256 of the stream and the stream behind its first 128 KiB),
    (d) on the device: the bytes are the emulator's."""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zstd_build as Z
import zstd_inspect as I
import zstd_parse as P
from zstd_build import LL, ML, OF

R = 4                      # SEQ_R of gc_zstd_seq.hip
N = 256 * R                # records (codes kernel) / sequences (pack kernel) per workgroup and round
G = 4 * N                  # merged sequences the ring holds
BLOCK = P.BLOCK_MAX
MAX_REC = BLOCK // 5 + 8   # GC_MAX_SEQ_PER_BLOCK
GOLDEN = os.path.join(HERE, "golden", "seq_rounds", "streams.npz")
RANDOM = np.random.default_rng(20261).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()
CAP = 6                    # records of a chain are this long: a chain of k records is a match of 6 * k bytes


def base():
    return P.Composer().lit(RANDOM).end_block(full=True)


def off_of(i):
    """the offset of plain sequence i: no two neighbours (or next-but-one neighbours) alike or one apart, all below 2^11"""
    return 40 + 5 * (i % 397)


def plain(c, i, ll=None, ml=4):
    """plain sequence i: 1 or 2 literals, a short match, an offset of its own"""
    ll = 1 + (i & 1) if ll is None else ll
    return c.lit(bytes([(i * 7 + k) & 255 for k in range(ll)])).match(ml, off_of(i))


def finish(c, tail=b"!"):
    return c.lit(tail).end_block()


# ---------------------------------------------------------------------------------------------- the cases: name -> function -> (composer, cap, checks on the frame)
CASES = {}


def case(name):
    def reg(fn):
        CASES[name] = fn
        return fn
    return reg


COUNTS = (1, R - 1, R, R + 1, N - 1, N, N + 1, 2 * N, 2 * N + 1, MAX_REC)


def _merged_count(n):
    """n sequences of one record each (no chains): as many merged sequences as raw records"""
    def fn():
        c = base()
        for i in range(n):
            plain(c, i, ml=40 if n < 64 else 3 + (i % 3 == 0), ll=None if n < 20000 else (i & 1))       # (a few short matches would not beat the block's raw form)
        return finish(c), CAP, lambda f: f.blocks[1].nseq == n
    return fn


def _raw_count(n):
    """n raw records: sequences of one, one and two records in turn (then whatever is left)"""
    def fn():
        c, left, i = base(), n, 0
        while left:
            k = min(left, (1, 1, 2)[i % 3])
            plain(c, i, ml={1: 40 if n < 64 else 3, 2: 9}[k], ll=None if n < 20000 else (i & 1))
            left -= k
            i += 1
        nseq = i
        return finish(c), CAP, lambda f: f.blocks[1].nseq == nseq
    return fn


for _n in COUNTS:
    CASES["merged_%d" % _n] = _merged_count(_n)
    CASES["raw_%d" % _n] = _raw_count(_n)


def _chain(lead, records, behind, tail=b"!"):
    """`lead` one-record sequences, one match of `records` records, `behind` more one-record sequences"""
    def fn():
        c = base()
        for i in range(lead):
            plain(c, i)
        c.lit(b"q").match(CAP * records, 131072)
        for i in range(lead + 1, lead + 1 + behind):
            plain(c, i)
        c = finish(c, tail)
        return c, CAP, lambda f: f.blocks[1].nseq == lead + 1 + behind and f.blocks[1].resolved[lead][:3] == (1, CAP * records, 131072)
    return fn


CASES.update({
    "chain_inside_a_thread": _chain(2 * R, R - 1, 5),                    # records 8, 9, 10
    "chain_fills_a_thread": _chain(2 * R, R, 5),                         # records 8 .. 11
    "chain_across_threads": _chain(2 * R - 2, R, 5),                     # records 6 .. 9
    "chain_over_a_whole_thread": _chain(R + 1, 3 * R, 5),                # records 5 .. 16: the thread of records 8 .. 11 and the next have no head
    "chain_across_waves": _chain(64 * R - 2, 5, 5),                      # records 254 .. 258
    "chain_across_rounds": _chain(N - 2, 5, 5),                          # records 1022 .. 1026
    "chain_ends_with_the_round": _chain(N - 5, 5, 5),                    # records 1019 .. 1023
    "chain_starts_the_round": _chain(N, 5, 5),
    "chain_of_more_than_a_round": _chain(N - 3, 2 * N + 9, 5),           # it is open over two whole rounds
    "chain_open_at_the_end": _chain(10, 7, 0, tail=b""),
    "chain_open_at_the_end_across_rounds": _chain(N - 4, 9, 0, tail=b""),
    "chain_behind_the_ring": _chain(G + 100, 10, 5),
    "chain_across_the_ring_edge": _chain(G - 2, 5, 20),                  # merged sequence G - 2, its records' lengths added where the ring wraps
    "chain_at_ring_slot_0": _chain(G, 2 * R + 1, 20),
})


@case("one_match_is_the_block")
def _():
    c = base().match(BLOCK, BLOCK).end_block(full=True)                    # 515 records of at most 255: one sequence
    return c, 255, lambda f: f.blocks[1].resolved == [(0, BLOCK, BLOCK, "new")]


@case("one_match_is_the_block_short_records")
def _():
    c = base().match(BLOCK, BLOCK).end_block(full=True)                    # 21 846 records: open over 21 rounds
    return c, CAP, lambda f: f.blocks[1].resolved == [(0, BLOCK, BLOCK, "new")]


def _run(first, last, behind=6):
    """plain sequences; those from `first` to `last` share one offset (with literals between them: rep1, not a chain), and the one behind the run has the
    offset of the one in front of it (rep2: the offset before the run, which the key scan carries over the run)"""
    def fn():
        c, n = base(), last + 1 + behind
        for i in range(n):
            if first <= i <= last:
                c.lit(bytes([i & 255])).match(4, 3001)
            elif i == last + 1 and first and behind:
                c.lit(b"xy").match(4, off_of(first - 1))
            else:
                plain(c, i)
        def ok(f):
            forms = [q[3] for q in f.blocks[1].resolved]
            return forms[first + 1:last + 1] == ["rep1"] * (last - first) and (not first or not behind or forms[last + 1] == "rep2") and f.blocks[1].nseq == n
        return finish(c), CAP, ok
    return fn


CASES.update({
    "run_inside_a_thread": _run(2 * R, 2 * R + 2),
    "run_across_threads": _run(2 * R - 2, 2 * R + 1),
    "run_over_a_whole_thread": _run(R + 1, 4 * R),
    "run_across_waves": _run(64 * R - 2, 64 * R + 2),
    "run_across_rounds": _run(N - 2, N + 2),
    "run_ends_with_the_round": _run(N - 5, N - 1),
    "run_starts_the_round": _run(N, N + 4),
    "run_of_more_than_a_round": _run(N - 3, 3 * N + 5),
    "run_from_the_first_sequence": _run(0, N + 1),
    "run_open_at_the_end": _run(N - 3, N + 9, behind=0),
    "run_across_the_ring_edge": _run(G - 2, G + 2),
})


def _ll0(at, form):
    """sequence `at` has no literals and the offset that makes `form` of it; the two in front of it set rep1 and rep2"""
    def fn():
        c, n = base(), at + 6
        a, b = 2500, 777
        for i in range(n):
            if i == at - 2:
                c.lit(b"ab").match(4, b)
            elif i == at - 1:
                c.lit(b"c").match(4, 1 if form == "rep1_is_1" else a)
            elif i == at:
                c.match(5, {"rep2": b, "rep1-1": a - 1, "rep1_is_1": 9, "new": 4000}[form])
            else:
                plain(c, i)
        want = {"rep2": "rep2", "rep1-1": "rep1-1", "rep1_is_1": "new", "new": "new"}[form]
        return finish(c), CAP, lambda f: f.blocks[1].resolved[at][3] == want and f.blocks[1].resolved[at][0] == 0 and f.blocks[1].nseq == n
    return fn


for _where, _at in (("thread", 2 * R), ("wave", 64 * R), ("round", N), ("second_round", 2 * N)):
    for _form in ("rep2", "rep1-1", "rep1_is_1", "new"):
        CASES["ll0_%s_first_of_a_%s" % (_form, _where)] = _ll0(_at, _form)


def _fat(nseq, places):
    """nseq plain sequences; the ones the pack kernel takes as its elements `places` (element u is sequence nseq - 1 - u) have long literal runs, long matches and the
    farthest offsets: the most bits a sequence of this frame can have, at the edges of a slab of 64, of a wave's R slabs, of a round"""
    def fn():
        c = base()
        fat = {nseq - 1 - u for u in places}
        lits = np.random.default_rng(nseq).integers(0, 256, 700 * len(places) + 8, dtype=np.uint8).tobytes()
        at = 0
        for i in range(nseq):
            if i in fat:
                c.lit(lits[at:at + 600 + i % 7]).match(1100 + i % 5, BLOCK + c.here() - (i % 3))
                at += 600 + i % 7
            else:
                plain(c, i)
        return finish(c), 255, lambda f: f.blocks[1].nseq == nseq and max(q[1] for q in f.blocks[1].codes) >= 16
    return fn


CASES.update({
    "fat_at_slab_and_wave_edges": _fat(N + 300, (0, 1, 63, 64, 65, 64 * R - 1, 64 * R, 64 * R + 1)),
    "fat_at_round_edges": _fat(2 * N + 300, (N - 2, N - 1, N, N + 1, 2 * N - 1, 2 * N)),
    "fat_last_of_a_short_round": _fat(N + 2, (N + 1, N, N - 1)),
})


@case("section_outgrows_its_block")
def _():
    """three 3-byte matches at far offsets: the section is longer than the 9 bytes it stands for, and the block is stored raw"""
    c = base()
    for off in (70001, 99999, 131072):
        c.match(3, off)
    c.end_block()
    return c, CAP, lambda f: [b.type for b in f.blocks] == ["raw", "raw"]


def _carry(seed):
    """two rounds and a bit of the pack kernel, with sequences whose bit counts differ (literal lengths with 0 to 3 extra bits): see test_carry_bits_take_every_value"""
    def fn():
        c, rng = base(), np.random.default_rng(1000 + seed)
        lls = rng.choice([1, 2, 17, 21, 23, 30], 2 * N + 40)
        for i, ll in enumerate(lls.tolist()):
            plain(c, i, ll=ll, ml=3 + int(rng.integers(0, 40)))
        return finish(c), CAP, lambda f: f.blocks[1].nseq == 2 * N + 40
    return fn


CARRY_SEEDS = (37, 4, 5, 1, 0, 10, 6, 15)          # (chosen among the first forty so that the carries 0, 1, .. 7 all occur; the test asserts that they do)
for _s in CARRY_SEEDS:
    CASES["carry_%d" % _s] = _carry(_s)


# ---------------------------------------------------------------------------------------------- running them
class Runner:
    def __init__(self, pkg, name, kw):
        self.name, self.enc, self.dec = name, pkg.ZstdEncoder(level=3, **kw), pkg.ZstdDecoder(**kw)

    def encode(self, x, blocks):
        cap = self.enc.compress_bound(x.size)
        if self.name == "gpu":
            import torch as t
            d_src, d_dst = t.from_numpy(np.array(x)).to("cuda:0"), t.full((cap,), 0xA5, dtype=t.uint8, device="cuda:0")
            t.cuda.synchronize()
            self.enc.code_parsed_device(d_src.data_ptr(), x.size, d_dst.data_ptr(), cap, blocks)
            return d_dst[:self.enc.finish()].cpu().numpy().tobytes()
        src, dst = np.ascontiguousarray(x), np.full(cap, 0xA5, np.uint8)
        self.enc.code_parsed_device(src.ctypes.data, x.size, dst.ctypes.data, cap, blocks)
        return dst[:self.enc.finish()].tobytes()

    def close(self):
        self.enc.close(); self.dec.close()


_EMU_BYTES = {}            # case -> the emulator's stream of this run (assertion (d))
_FRAMES = {}               # case -> the inspector's frame (test_carry_bits_take_every_value)


def emu_stream(pkg, lib_path, name):
    """the stream of one case from an emulator library (tools/record_seq_rounds.py records the golden file with this)"""
    c, cap, _ = CASES[name]()
    x = c.x()
    r = Runner(pkg, "emu", dict(lib_path=lib_path))
    try:
        return r.encode(x, P.rows(x, c.blocks, cap))
    finally:
        r.close()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k[4:]: (z[k].tobytes(), z["tail_" + k[4:]].tobytes()) for k in z.files if k.startswith("sha_")}


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


def run_case(T, O, golden, name):
    comp, cap, ok = CASES[name]()
    x = comp.x()
    blocks = P.rows(x, comp.blocks, cap)
    s = T.encode(x, blocks)
    if T.name == "emu":
        _EMU_BYTES[name] = s
    else:
        if name not in _EMU_BYTES:
            _EMU_BYTES[name] = T.emu.encode(x, blocks)
        assert s == _EMU_BYTES[name], "%s: the device's bytes differ from the emulator's" % name                     # (d)
    sha, tail = golden[name]
    assert hashlib.sha256(s).digest() == sha and s[BLOCK:] == tail, "%s: not the bytes of the commit in front of the rounds" % name      # (c)
    a = np.frombuffer(s, dtype=np.uint8)
    assert np.array_equal(O.port_zstd_decompress(a, x.size), x), "%s: the oracle's decoder" % name                    # (a)
    if O.ref("zstd") is not None:
        assert np.array_equal(O.ref_zstd_decompress(a, x.size), x), "%s: the reference's decoder" % name
    assert np.array_equal(T.dec.code(a), x), "%s: this project's decoder" % name
    frames = I.inspect(s)
    assert len(frames) == 1 and frames[0].content == x.tobytes() and len(frames[0].blocks) == len(comp.blocks)
    for b, (blk, (_, n, seqs)) in enumerate(zip(frames[0].blocks, comp.blocks)):                                      # (b)
        assert len(blk.content) == n
        if blk.type == "raw":
            continue
        got, want = [q[:3] for q in blk.resolved], P.merged(seqs)
        assert len(got) == len(want) == blk.nseq, "%s: block %d has %d sequences, the parse %d" % (name, b, len(got), len(want))
        if got != want:
            k = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError("%s: block %d sequence %d is %r, the parse says %r" % (name, b, k, got[k], want[k]))
    assert ok(frames[0]), "%s: the case does not show what it is named after" % name
    _FRAMES[name] = frames[0]
    return frames[0]


@pytest.mark.parametrize("name", sorted(k for k in CASES if not k.startswith("carry_")))
def test_round_edges(T, O, golden, name):
    run_case(T, O, golden, name)


def test_carry_bits_take_every_value(T, O, golden):
    """the bits a round leaves over for the next one's first byte: the cases carry_* differ in the bit counts of their sequences; between them the first round edge
    sees every carry from 0 to 7.  The carry is read off the stream: the bitstream's length in bits minus what the sequences in front of the last N take, which the
    inspector's codes and a walk of its tables' states give."""
    seen = set()
    for s in CARRY_SEEDS:
        name = "carry_%d" % s
        f = run_case(T, O, golden, name)
        blk = f.blocks[1]
        assert blk.nseq == 2 * N + 40
        seen.add(_first_round_bits(_EMU_BYTES[name], blk) & 7)
    assert seen == set(range(8)), "carries seen at the first round edge: %r" % sorted(seen)


def _first_round_bits(stream, blk):
    """bits of the last N sequences of the block = what the pack kernel's first round writes.  The decoder reads the bitstream backwards: the three start states, then
    per sequence its extra bits and (but behind the last) the bits of the three state steps.  A walk with the tables the inspector read gives every count."""
    tabs = []
    for w in (LL, OF, ML):
        if blk.modes[w] == Z.MODE_RLE:
            tabs.append(Z.FseTable.of_rle(blk.rle_syms[w]))
        elif blk.modes[w] == Z.MODE_PREDEFINED:
            tabs.append(Z.FseTable(*Z.DEFAULTS[w]))
        else:
            tabs.append(Z.FseTable(blk.norms[w], blk.logs[w]))
    # the block is the last thing in the stream and the bitstream the last thing in the block: read backwards, the bytes in front of it do not matter
    payload = stream[len(stream) - blk.seq_section_bytes:]
    r = I.BackReader(payload)
    st = [0, 0, 0]
    for w in (LL, OF, ML):
        st[w] = r.read(tabs[w].log)
    per = []
    for i in range(blk.nseq):
        before = r.pos
        llc, ofc, mlc = tabs[LL].sym[st[LL]], tabs[OF].sym[st[OF]], tabs[ML].sym[st[ML]]
        assert (llc, ofc, mlc) == blk.codes[i]
        r.read(ofc); r.read(Z.ML_BITS[mlc]); r.read(Z.LL_BITS[llc])
        if i + 1 < blk.nseq:
            for w in (LL, ML, OF):
                st[w] = tabs[w].base[st[w]] + r.read(tabs[w].nb[st[w]])
        per.append(before - r.pos)
    assert r.pos >= 0 and r.pos % 8 == 0            # (what is left is the section's header)
    return sum(per[-N:])
