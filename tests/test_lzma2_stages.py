"""The LZMA2 encoder's back end -- L1 gc_lzma2_prep_kernel (item lists), L2 gc_lzma2_model_kernel, L3 gc_lzma2_rc_kernel / gc_lzma2_rc_fin_kernel (gc_lzma2_enc.hip), the
segment-kind, plan and emit kernels (gc_lzma2_frame.hip) and the launches they share with the stream call (gc_api.hip flzma2_stage / flzma2_code_part /
flzma2_join_and_emit) -- on EXACT parses, one named case per branch.  The test entry gc_test_flzma2_encode_parsed (test builds only) takes the records the match finder
would have left and the parse's window costs, so a case decides which items the kernels get; tests/lzma2_parse.py composes the input and says which match-type symbols must
come out; tests/lzma2_inspect.py (an LZMA2 reader written from the format) says what the encoder wrote.  Every parsed case asserts

    (a) the stream decodes to the input under the plain-C decoder of the oracle, the reference's decoder (where oracle/_ref is built) and this project's decoder,
    (b) the match-type symbols the inspector reads -- position, kind, length, distance -- are exactly lzma2_parse.expected(...), and the content is the input,
    (c) the inspector shows the branch the case is named after,
    (d) on the device: the bytes are the emulator's.

A case is two blocks as a rule: 128 KiB of random bytes given a window cost of 8 bits per byte (L2 stores it unmodelled; it is the history the matches copy from), then
the block under test, short and last.  The word-level tests feed L3 (probability, bit) words of their own (gc_test_lzma2_rc_words) and compare every byte with a
classical cache-and-pending range coder written here.

Found unreachable (and therefore not a case):
  * one message for "in front of its frame" and "beyond the level's dictionary": a frame is never longer than the dictionary the level states (8 MiB / 16 MiB), so the
    second can only fire alone in a group of overlapping frames, i.e. in an input of more than 8 MiB -- the entry checks both, one refusal stands for them.
  * carry into the first byte of a chunk: the coder's interval starts below 2^32, so byte 0 is always 0 (the decoders insist on it, and every case decodes)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lzma2_inspect as I
import lzma2_parse as P
from lzma2_inspect import LIT, MLIT, MATCH, SHORTREP, REP0, REP1, REP2, REP3

BLOCK, RC = P.BLOCK_MAX, P.RC
R = np.random.default_rng(20261).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()      # block 0 of most cases
MAX_SEQ = BLOCK // 5 + 8                                                                 # GC_MAX_SEQ_PER_BLOCK
HOPELESS, CHEAP = 128, 4                                                                 # window costs per byte in 1/16 bit: 8 bits per byte; a quarter of a bit per byte
SEG_LOG = {1: 14, 3: 15, 5: 17, 7: 17}


def costs(comp, per_byte):
    """the parse's estimate per 4 KiB window of every block (32 words each): per_byte[b] for every byte of block b that the window holds"""
    wc = np.zeros((len(comp.blocks), 32), np.uint32)
    for b, (_, n, _) in enumerate(comp.blocks):
        for w in range(32):
            wc[b, w] = max(0, min(RC, n - w * RC)) * per_byte[b]
    return wc


def rnd(n, seed):
    """filler literals of the blocks under test: four letters at random, two bits each, so that a block of them and a few matches is coded, not stored"""
    return np.frombuffer(b"acgt", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


# ---------------------------------------------------------------------------------------------- the two backends
class Runner:
    def __init__(self, pkg, name, kw):
        self.name, self.pkg, self.kw = name, pkg, kw
        self.enc, self.dec = pkg.Flzma2Encoder(level=5, **kw), pkg.Lzma2Decoder(**kw)
        if name == "gpu":
            import torch
            self.torch = torch

    def encode(self, x, blocks, level=5, win_cost=None, flags=0):
        self.enc.set_level(level)
        cap = self.enc.compress_bound(x.size)
        if self.name == "gpu":
            t = self.torch
            d_src, d_dst = t.from_numpy(np.array(x)).to("cuda:0"), t.full((cap,), 0xA5, dtype=t.uint8, device="cuda:0")
            t.cuda.synchronize()
            self.enc.code_parsed_device(d_src.data_ptr(), x.size, d_dst.data_ptr(), cap, blocks, win_cost, flags)
            return d_dst[:self.enc.finish()].cpu().numpy().tobytes()
        src, dst = np.ascontiguousarray(x), np.full(cap, 0xA5, np.uint8)
        self.enc.code_parsed_device(src.ctypes.data, x.size, dst.ctypes.data, cap, blocks, win_cost, flags)
        return dst[:self.enc.finish()].tobytes()

    def prop(self, level):
        self.enc.set_level(level)
        return self.enc.coder_props()[0]

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


def same_as_emulator(T, name, got, again):
    if T.name == "emu":
        _EMU_BYTES[name] = got
        return
    if name not in _EMU_BYTES:
        _EMU_BYTES[name] = again(T.emu)
    assert got == _EMU_BYTES[name], "%s: the device's bytes differ from the emulator's" % name                         # (d)


def check(T, O, name, comp, level=5, win_cost="history", flags=0, rep4=True, leaders=None, stored=None):
    """assertions (a), (b), (d) on a composed input -> (the inspector's stream, its symbols as a {position: Symbol})"""
    x = comp.x()
    blocks = P.rows(x, comp.blocks)
    seg_log = SEG_LOG[level]
    if isinstance(win_cost, str):                                   # block 0 hopeless, the others cheap
        win_cost = costs(comp, [HOPELESS] + [CHEAP] * (len(blocks) - 1))
        stored = set(range(BLOCK >> seg_log)) if stored is None else stored
    stored = stored or ()
    s = T.encode(x, blocks, level, win_cost, flags)
    same_as_emulator(T, name, s, lambda emu: emu.encode(x, blocks, level, win_cost, flags))
    prop = T.prop(level)
    body = s if not (flags & 1) else s + b"\x00"
    a = np.frombuffer(body, dtype=np.uint8)
    assert np.array_equal(O.port_lzma2_decode(a, x.size, prop), x), "%s: the oracle's decoder" % name                  # (a)
    if O.ref("flzma2") is not None:
        assert np.array_equal(O.ref_lzma2_decode(a, x.size, prop), x), "%s: the reference's decoder" % name
    assert np.array_equal(T.dec.code(a, prop), x), "%s: this project's decoder" % name
    st = I.inspect(s, dict_size=(2 | (prop & 1)) << (prop // 2 + 11), need_end_mark=not (flags & 1))
    assert st.content == x.tobytes(), "%s: the inspector's content" % name                                            # (b)
    got = [(q.pos, q.kind, q.length, q.dist) for q in I.symbols(st) if q.kind not in (LIT, MLIT)]
    want = P.expected(comp.blocks, seg_log, rep4, leaders, stored)
    if got != want:
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError("%s: symbol %d is %r, the parse says %r (%d symbols, %d expected)" % (name, k, got[k] if k < len(got) else None,
                                                                                                   want[k] if k < len(want) else None, len(got), len(want)))
    return st, {q.pos: q for q in I.symbols(st)}


def hist():
    return P.Composer().lit(R).end_block(full=True)


def to(c, pos, seed=1):
    """random literals up to block position pos"""
    assert pos >= c.here()
    return c.lit(rnd(pos - c.here(), seed * 1000 + pos))


def lz_chunks(st, pos0=0):
    return [c for c in st.chunks if c.control >= 0x80 and c.pos >= pos0]


# ---------------------------------------------------------------------------------------------- the cases: name -> (composer, check arguments, assertion (c))
CASES = {}


def case(name, **kw):
    def deco(fn):
        assert name not in CASES
        CASES[name] = (fn, kw)
        return fn
    return deco


def _len_case(ml, want):
    def build():
        c = to(hist(), 100).match(ml, 70001)
        return to(c, c.here() + 50, 2).end_block()

    def shows(st, sym, x):
        got, p = [], BLOCK + 100
        while p in sym and sym[p].kind in (MATCH, REP0) and len(got) < len(want):
            got.append(sym[p].length)
            p += sym[p].length
        assert got == want and sym[BLOCK + 100].kind == MATCH and all(sym[BLOCK + 100 + sum(want[:i])].kind == REP0 for i in range(1, len(want)))
    return build, shows


for _ml, _want in ((255, [255]), (256, [256]), (550, [273, 273, 4]), (273, [273]), (274, [272, 2]), (275, [273, 2]), (546, [273, 273]), (547, [273, 272, 2])):
    _b, _s = _len_case(_ml, _want)
    CASES["l1_len_%d" % _ml] = (lambda b=_b, s=_s: (b(), s), {})


@case("l1_over_boundaries")
def _():
    c = to(hist(), 3000).match(10000, 99999)
    def shows(st, sym, x):
        assert [sym[BLOCK + p].pos for p in (3000, 4096, 8192, 12288)] and sym[BLOCK + 4096].kind == REP0 and sym[BLOCK + 12288 + 273 * 2].length == 712 - 546
    return to(c, 13100, 2).end_block(), shows


@case("l1_ends_one_past_boundary")
def _():
    c = to(hist(), 4000).match(97, 5000)
    def shows(st, sym, x):
        assert sym[BLOCK + 4000].length == 96 and sym[BLOCK + 4096].kind == MLIT
    return to(c, 4200, 2).end_block(), shows


@case("l1_starts_one_before_boundary")
def _():
    c = to(hist(), 4095).match(50, 5000)
    def shows(st, sym, x):
        assert sym[BLOCK + 4095].kind == LIT and sym[BLOCK + 4096].kind == MATCH and sym[BLOCK + 4096].length == 49
    return to(c, 4200, 2).end_block(), shows


@case("l1_one_byte_at_both_ends")
def _():
    c = to(hist(), 4095).match(4098, 5000)
    def shows(st, sym, x):
        assert sym[BLOCK + 4095].kind == LIT and sym[BLOCK + 4096].kind == MATCH and sym[BLOCK + 8192].kind == MLIT
    return to(c, 8300, 2).end_block(), shows


@case("l1_two_bytes_astride_short_rep")
def _():
    c = to(hist(), 4000).match(20, 777)
    to(c, 4095, 2).match(2, 777)
    def shows(st, sym, x):
        assert sym[BLOCK + 4095].kind == LIT and sym[BLOCK + 4096].kind == SHORTREP
    return to(c, 4200, 3).end_block(), shows


@case("l1_two_bytes_astride_literal")
def _():
    c = to(hist(), 4000).match(20, 777)
    to(c, 4095, 2).match(2, 778)
    def shows(st, sym, x):
        assert sym[BLOCK + 4095].kind == LIT and sym[BLOCK + 4096].kind == LIT
    return to(c, 4200, 3).end_block(), shows


@case("l1_literal_runs")
def _():
    c = to(hist(), 10)
    for k, run in enumerate((0, 15, 16, 17, 33)):
        c.match(5, 1000 + k).lit(rnd(run, 50 + k))
    c.match(5, 2000)
    def shows(st, sym, x):
        p = BLOCK + 10
        for run in (0, 15, 16, 17, 33):
            assert sym[p].kind == MATCH and all(sym[p + 5 + i].kind in (LIT, MLIT) for i in range(run)) and sym[p + 5 + run].kind == MATCH
            p += 5 + run
    return c.lit(rnd(7, 60)).end_block(), shows


@case("l1_literal_run_ends_on_boundary")
def _():
    c = to(hist(), 4096).match(30, 4000)
    def shows(st, sym, x):
        assert sym[BLOCK + 4095].kind == LIT and sym[BLOCK + 4096].kind == MATCH and [(ch.pos, ch.control) for ch in lz_chunks(st, BLOCK)] == [(BLOCK, 0xC0), (BLOCK + RC, 0x80)]
    return to(c, 4200, 2).end_block(), shows


@case("l1_no_records")
def _():
    def shows(st, sym, x):
        assert all(q.kind == LIT for q in sym.values()) and len(sym) == 3000
    return to(hist(), 3000).end_block(), shows


@case("l1_ends_in_match")
def _():
    c = to(hist(), 500).match(300, 131000)
    def shows(st, sym, x):
        assert sym[BLOCK + 500 + 273].length == 27 and BLOCK + 800 == len(st.content)
    return c.end_block(), shows


@case("l1_starts_with_match_into_history")
def _():
    c = hist().match(40, 70000)
    def shows(st, sym, x):
        q = sym[BLOCK]
        assert (q.kind, q.length, q.dist, q.state) == (MATCH, 40, 70000, 0)
    return to(c, 100, 2).end_block(), shows


@case("l1_last_block_of_1", win_cost="cheap", leaders={0})          # (a block this short is coded only as the tail of a merged segment: on its own it is stored)
def _():
    def shows(st, sym, x):
        assert sym[BLOCK].kind == MLIT and len(st.content) == BLOCK + 1
    return _cheap_blocks(1, 0).lit(b"\x42").end_block(), shows


@case("l1_last_block_of_2", win_cost="cheap", leaders={0})
def _():
    def shows(st, sym, x):
        assert sym[BLOCK].length == 2 and sym[BLOCK].kind == MATCH and len(st.content) == BLOCK + 2
    return _cheap_blocks(1, 0).match(2, 77).end_block(), shows


@case("l1_last_block_of_17", win_cost="cheap", leaders={0})
def _():
    def shows(st, sym, x):
        assert sym[BLOCK + 3].length == 14 and sym[BLOCK + 3].kind == MATCH and len(st.content) == BLOCK + 17
    return _cheap_blocks(1, 0).lit(b"abc").match(14, 9).end_block(), shows


@case("l1_densest_block_is_stored", stored={0, 1})
def _():
    c = hist()
    for i in range(BLOCK // 5):
        c.lit(rnd(3, 7000 + i) if i < 4 else bytes([i & 255, (i >> 8) & 255, (i * 7) & 255])).match(2, 100000 + (i % 30000))
    c.lit(b"zz")
    def shows(st, sym, x):
        assert not sym and all(ch.control in (1, 2) for ch in st.chunks)
    return c.end_block(full=True), shows


# ---- L2: kinds and history
@case("l2_every_kind")
def _():
    c = to(hist(), 20)
    for d in (1001, 1002, 1003, 1004):
        c.match(6, d).lit(rnd(2, d))
    for d in (1001, 1002, 1002, 1004, 1003):                          # rep3, rep3, rep0, rep2, rep3
        c.match(7, d).lit(rnd(1, d + 10))
    c.match(1, 1003)
    def shows(st, sym, x):
        kinds = [q.kind for q in sym.values() if q.kind not in (LIT, MLIT)]
        assert kinds == [MATCH] * 4 + [REP3, REP3, REP0, REP2, REP3, SHORTREP], kinds
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_rep1_rep2_named")
def _():
    c = to(hist(), 20)
    for d in (1001, 1002, 1003):
        c.match(6, d).lit(rnd(2, d))
    c.match(5, 1002).lit(b"q").match(5, 1001)                         # rep1, then 1001 at index 2 of (1002, 1003, 1001, 1)
    def shows(st, sym, x):
        kinds = [q.kind for q in sym.values() if q.kind not in (LIT, MLIT)]
        assert kinds == [MATCH] * 3 + [REP1, REP2], kinds
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_one_byte_behind_literal_is_literal")
def _():
    c = to(hist(), 20).match(9, 500).lit(rnd(3, 9)).match(1, 600)
    def shows(st, sym, x):
        assert sym[BLOCK + 32].kind == LIT and sym[BLOCK + 32].state == 0
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_one_byte_behind_match_is_matched_literal")
def _():
    c = to(hist(), 20).match(9, 500).match(1, 600)
    def shows(st, sym, x):
        assert sym[BLOCK + 29].kind == MLIT and sym[BLOCK + 29].state == 7 and sym[BLOCK + 29].dist == 500
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_rep4_off_rep2_rep3_are_matches", rep4=False, env={"GC_L2_REP4": "0"})
def _():
    c = to(hist(), 20)
    for d in (1001, 1002, 1003, 1004):
        c.match(6, d).lit(rnd(2, d))
    c.match(7, 1001).lit(b"x").match(7, 1003).lit(b"y").match(7, 1001).lit(b"z").match(7, 1001)
    def shows(st, sym, x):
        kinds = [q.kind for q in sym.values() if q.kind not in (LIT, MLIT)]
        assert kinds == [MATCH] * 6 + [REP1, REP0], kinds
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_rep4_off_one_byte_items_in_a_later_tile", rep4=False, env={"GC_L2_REP4": "0"})
def _():
    c = to(hist(), 20).match(6, 777).lit(rnd(16 * 70, 5))             # 70 cut items on, in the second tile of 64 items: the repeat distance is still 777
    c.match(1, 777).lit(rnd(5, 6)).match(1, 1).lit(rnd(5, 7)).match(1, 777)
    def shows(st, sym, x):
        p = BLOCK + 26 + 16 * 70
        assert [sym[q].kind for q in (p, p + 6, p + 12)] == [SHORTREP, LIT, SHORTREP]
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_repeats_far_back_in_items")
def _():
    c = to(hist(), 20).match(6, 3001).lit(b"a").match(6, 3002)
    c.lit(rnd(16 * 70, 5)).match(6, 3001)                             # rep1, 70 cut items behind its last use
    c.lit(rnd(16 * 130, 6)).match(6, 3002)                            # rep1 again, 130 cut items on
    c.lit(rnd(16 * 200, 7)).match(6, 3002).lit(rnd(16 * 66, 8)).match(1, 3002)
    def shows(st, sym, x):
        kinds = [q.kind for q in sym.values() if q.kind not in (LIT, MLIT)]
        assert kinds == [MATCH, MATCH, REP1, REP1, REP0, SHORTREP], kinds
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_rotation_across_tile_boundary")
def _():
    c = to(hist(), 16 * 58 + 3)                                       # 58 cut items in front: the twelve matches are items 58 .. 69
    for d in (2001, 2002, 2003, 2004) * 3:
        c.match(4, d)
    def shows(st, sym, x):
        kinds = [q.kind for q in sym.values() if q.kind not in (LIT, MLIT)]
        assert kinds == [MATCH] * 4 + [REP3] * 8, kinds
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_list_carried_into_a_tile_and_reordered")
def _():
    c = to(hist(), 16 * 58 + 3)                                       # items 58 .. 63 leave (2002, 2001, 2004, 2003) to the next tile
    for d in (2001, 2002, 2003, 2004, 2001, 2002):
        c.match(4, d)
    for d in (2001, 2003, 2004):                                      # ... where 2001 comes out of its MIDDLE: 2003 and 2004 are rep3 only if it was taken out, not just put in front
        c.match(4, d)
    def shows(st, sym, x):
        kinds = [q.kind for q in sym.values() if q.kind not in (LIT, MLIT)]
        assert kinds == [MATCH] * 4 + [REP3, REP3, REP1, REP3, REP3], kinds
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_distance_1_first_is_rep0")
def _():
    c = to(hist(), 20).match(8, 1)
    def shows(st, sym, x):
        assert sym[BLOCK + 20].kind == REP0
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_distance_1_second_is_rep1")
def _():
    c = to(hist(), 20).match(8, 555).lit(b"k").match(8, 1)
    def shows(st, sym, x):
        assert sym[BLOCK + 29].kind == REP1 and sym[BLOCK + 29].dist == 1
    return c.lit(rnd(5, 3)).end_block(), shows


@case("l2_short_rep_second_symbol", win_cost=None)
def _():
    c = P.Composer().lit(b"a").match(1, 1)
    def shows(st, sym, x):
        assert st.chunks[0].symbols[1].kind == SHORTREP and st.chunks[0].symbols[1].state == 0 and st.chunks[0].control == 0xE0
    return c.lit(rnd(40, 3)).match(400, 4).end_block(), shows                  # (the long match: without it the block is stored)


def _astride_segment(level, seg):
    def build():
        c = P.Composer().lit(rnd(seg - 4, 70 + level)).match(100, 3000)
        def shows(st, sym, x):
            assert sym[seg - 4].kind == MATCH and sym[seg].kind == MATCH and sym[seg].state == 0 and sym[seg].length == 96
            assert [ch.control for ch in st.chunks if ch.pos == seg] == [0xC0]
        return c.lit(rnd(300, 71)).end_block(), shows
    return build


CASES["l2_match_astride_segment_level_1"] = (_astride_segment(1, 1 << 14), dict(level=1, win_cost=None))
CASES["l2_match_astride_segment_level_3"] = (_astride_segment(3, 1 << 15), dict(level=3, win_cost=None))


@case("l2_match_astride_rc_boundary")
def _():
    c = to(hist(), 4090).match(100, 3000)
    def shows(st, sym, x):
        assert sym[BLOCK + 4090].kind == MATCH and sym[BLOCK + 4096].kind == REP0 and sym[BLOCK + 4096].length == 94
    return to(c, 4300, 2).end_block(), shows


def _two_cheap_blocks():
    c = P.Composer().lit(rnd(64, 80))
    while c.here() < BLOCK:
        c.match(min(4000, BLOCK - c.here()), 64)
    c.end_block(full=True)
    return c.match(3000, 64).lit(rnd(9, 81)).end_block()


@case("l2_same_distance_across_blocks_merged", win_cost="cheap", leaders={0})
def _():
    def shows(st, sym, x):
        assert sym[BLOCK].kind == REP0 and [ch.control for ch in st.chunks if ch.pos >= BLOCK] == [0x80]
    return _two_cheap_blocks(), shows


@case("l2_same_distance_across_blocks_unmerged", win_cost="cheap", env={"GC_SEG_MERGE": "0"})
def _():
    def shows(st, sym, x):
        assert sym[BLOCK].kind == MATCH and [ch.control for ch in st.chunks if ch.pos >= BLOCK] == [0xC0]
    return _two_cheap_blocks(), shows


# ---- L2: probabilities
@case("l2_run_of_equal_literals")
def _():
    def shows(st, sym, x):
        assert len(sym) == 2000
    return hist().lit(b"\x00" * 2000).end_block(), shows


@case("l2_probabilities_sharing_a_ticket")
def _():
    # A probability's ticket byte is its index mod 2048.  The length coder's choice bit (index 144) shares one with 144 + 2048 -- the literal coder's node 44 (the five
    # bits 01100 read) in context 1 (previous byte 0x20..0x3F): an 'a' behind a space -- and with 144 + 4096: context 3 (previous byte 0x60..0x7F), node 44 of the
    # matched-literal tree's "match bit 1" half: an 'a' right behind a match that ends in 'u' where the match would have gone on with 'e'.  Every unit below has all three
    # -- a match at a fresh distance, the matched 'a', a space, the plain 'a' -- within some 45 events, so they meet in the 64-event steps.
    c = to(hist(), 8).lit(b"zue ")
    for k in range(150):
        c.match(2, 4 + 5 * k).lit(b"a a")
    def shows(st, sym, x):
        m = [q for q in sym.values() if q.kind == MATCH]
        assert len(m) == 150 and all(sym[q.pos + 2].kind == MLIT and x[q.pos + 2] == 0x61 and x[q.pos + 2 - q.dist] == 0x65 and sym[q.pos + 4].kind == LIT for q in m)
    return c.lit(rnd(9, 3)).end_block(), shows


@case("l2_tile_needs_several_event_rounds")
def _():
    c = to(hist(), 16)
    for i in range(70):                                              # 64 items of 16 literals + a far match: 144 + ~40 events each, 1600 fit a round
        c.match(3, 90000 + i * 17).lit(rnd(16, 900 + i))
    def shows(st, sym, x):
        assert sum(1 for q in sym.values() if q.kind == MATCH) == 70
    return c.end_block(), shows


@case("l2_item_with_most_events")
def _():
    c = to(hist(), 16).match(200, 131072 + 16).lit(rnd(16, 4))
    c.match(18, BLOCK + c.here())      # 16 literals, then: len >= 18 (high tree), the farthest distance (direct bits + align)
    def shows(st, sym, x):
        q = sym[BLOCK + 232]
        assert q.kind == MATCH and q.length == 18 and q.dist == BLOCK + 232
    return c.lit(rnd(5, 3)).end_block(), shows


# ---- L2: props
@case("props_short_segment_keeps_lc3", win_cost=None)
def _():
    body = np.arange(1000, dtype="<u4").tobytes()[:4000]
    def shows(st, sym, x):
        assert st.chunks[0].props == (3, 0, 2) and st.chunks[0].control == 0xE0
    return P.Composer().lit(body).end_block(), shows


@case("props_text_lc3", win_cost=None)
def _():
    words = [b"the ", b"quick ", b"brown ", b"fox ", b"jumps ", b"over ", b"lazy ", b"dog. ", b"And ", b"then "]
    g = np.random.default_rng(5)
    body = b"".join(words[i] for i in g.integers(0, len(words), 2000))[:8192]
    def shows(st, sym, x):
        assert st.chunks[0].props == (3, 0, 2)
    return P.Composer().lit(body).end_block(), shows


@case("props_two_byte_fields_lc2_lp1", win_cost=None)
def _():
    g = np.random.default_rng(6)
    a = np.zeros(8192, np.uint8)
    a[0::2] = g.integers(0, 256, 4096)                               # low bytes random, high bytes from a small set that the position predicts and the previous byte does not
    a[1::2] = g.integers(0, 4, 4096) * 64 + 1
    def shows(st, sym, x):
        assert st.chunks[0].props == (2, 1, 2)
    return P.Composer().lit(a.tobytes()).end_block(), shows


@case("props_four_byte_records_lc0_lp2", win_cost=None)
def _():
    g = np.random.default_rng(7)
    a = np.zeros(8192, np.uint8)
    for k, (lo, n) in enumerate(((0, 256), (0x10, 3), (0x80, 3), (0xF0, 3))):
        a[k::4] = g.integers(0, n, 2048) + lo
    def shows(st, sym, x):
        assert st.chunks[0].props == (0, 2, 2)
    return P.Composer().lit(a.tobytes()).end_block(), shows


# ---- segments and chunks
def _cheap_blocks(n_full, last, dist=64, seed=90):
    c = P.Composer().lit(rnd(dist, seed))
    for b in range(n_full):
        while c.here() < BLOCK:
            c.match(min(4096 - c.here() % 4096, BLOCK - c.here()), dist)
        c.end_block(full=True)
    if last:
        c.match(last, dist).end_block()
    return c


@case("seg_rc_chunks_merged_into_one", win_cost=None)
def _():
    def shows(st, sym, x):
        ch = lz_chunks(st)
        assert len(ch) == 1 and ch[0].usize == BLOCK and ch[0].control == 0xE1
    return _cheap_blocks(1, 0), shows


def _third_literal_block():
    """eight rc chunks of about 11 900 words each: 1 300 literals (9 words a byte) and a match over the other 2 796 bytes"""
    c = P.Composer()
    for k in range(8):
        c.lit(rnd(1300, 100 + k)).match(2796, 1300 if k == 0 else 4096)
    return c.end_block()


@case("seg_merge_words_level_5", win_cost=None)
def _():
    def shows(st, sym, x):
        assert [ch.usize for ch in lz_chunks(st)] == [2 * RC] * 4               # two chunks stay within 32 768 words, three do not
    return _third_literal_block(), shows


@case("seg_merge_words_level_7", win_cost=None, level=7)
def _():
    def shows(st, sym, x):
        assert [ch.usize for ch in lz_chunks(st)] == [4 * RC] * 2               # four stay within 49 152
    return _third_literal_block(), shows


def _groups(n_blocks, last, leaders, cost=None, **kw):
    def build():
        def shows(st, sym, x):
            heads = sorted(ch.pos // BLOCK for ch in st.chunks if ch.control >= 0xC0)
            assert heads == sorted(leaders), heads
            assert all(ch.props is not None for ch in lz_chunks(st))
        return _cheap_blocks(n_blocks, last), shows
    return build, dict(win_cost="cheap" if cost is None else cost, leaders=set(leaders), **kw)


CASES["seg_group_of_2"] = _groups(2, 0, [0])
CASES["seg_group_of_4"] = _groups(4, 0, [0])
CASES["seg_group_of_8"] = _groups(8, 0, [0])
CASES["seg_three_blocks_two_plus_one"] = _groups(3, 0, [0, 2])
CASES["seg_short_last_block_in_group"] = _groups(3, 5000, [0])
CASES["seg_budget_splits_four_into_twos"] = _groups(4, 0, [0, 2], cost=lambda c: costs(c, [16 * 655360 // (2 * BLOCK)] * 4))     # two blocks fit the budget (16 x 655 360), four do not


@case("seg_hopeless_block_between_cheap_ones", win_cost=lambda c: costs(c, [CHEAP, HOPELESS, CHEAP, CHEAP]), leaders={0, 1, 2}, stored={1})
def _():
    def shows(st, sym, x):
        assert all(ch.control == 2 for ch in st.chunks if BLOCK <= ch.pos < 2 * BLOCK)
        assert sorted(ch.pos // BLOCK for ch in st.chunks if ch.control >= 0xC0) == [0, 2]
    return _cheap_blocks(4, 0), shows


@case("seg_no_end_mark", flags=1)
def _():
    def shows(st, sym, x):
        assert not st.end_mark
    return to(hist(), 100).match(50, 1000).lit(b"end").end_block(), shows


@case("seg_stored_then_coded")
def _():
    def shows(st, sym, x):
        assert st.chunks[0].control == 1 and [ch.control for ch in st.chunks if ch.pos == BLOCK] == [0xC0] and st.chunks[-1].props == (3, 0, 2)
    return to(hist(), 100).match(50, 1000).lit(b"end").end_block(), shows


N_CASES = 60


def test_case_list():
    assert len(CASES) == N_CASES, sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_parsed(T, O, name, monkeypatch):
    build, kw = CASES[name]
    kw = dict(kw)
    for k, v in kw.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    comp, shows = build()
    wc = kw.get("win_cost", "history")
    if wc == "cheap":
        kw["win_cost"] = costs(comp, [CHEAP] * len(comp.blocks))
    elif callable(wc):
        kw["win_cost"] = wc(comp)
    st, sym = check(T, O, name, comp, **kw)
    shows(st, sym, comp.x())                                                                                           # (c)


# ---------------------------------------------------------------------------------------------- overflow inside a merged segment
@pytest.mark.parametrize("which", [0, 1, 3])
def test_overflow_in_merged_segment_stores_it_whole(T, O, which, monkeypatch):
    """four cheap blocks in one model segment; block `which` is the densest parse there is (two-byte far matches, three literals between them: 10.8 words per byte), its words
    outgrow their place, and the WHOLE segment is stored; the segment behind it (a fifth block) starts with a state reset"""
    c = P.Composer().lit(rnd(64, 90))
    for b in range(5):
        if b == which:
            for i in range((BLOCK - c.here()) // 5):
                c.lit(bytes([i & 255, (i >> 8) & 255, (i * 7) & 255])).match(2, len(c.out) - (i % 50))      # as far back as the input goes: 39 words and the distance's footer
            c.lit(b"z" * (BLOCK - c.here()))
        elif b < 4:
            while c.here() < BLOCK:
                c.match(min(4096 - c.here() % 4096, BLOCK - c.here()), 64)
        else:
            c.match(3000, 64)
        c.end_block(full=b < 4)
    st, sym = check(T, O, "overflow_%d" % which, c, win_cost=costs(c, [CHEAP] * 5), leaders={0, 4}, stored={0, 1, 2, 3})
    assert all(ch.control in (1, 2) for ch in st.chunks if ch.pos < 4 * BLOCK)
    assert [ch.control for ch in st.chunks if ch.pos >= 4 * BLOCK] == [0xC0] and sym[4 * BLOCK].kind == MATCH


# ---------------------------------------------------------------------------------------------- L2: states, lengths, distances
def test_every_state_in_front_of_literals_and_matches(T, O):
    """M = match, R = rep0, Q = the rep0 that the cut at 273 makes of a long match's rest, S = short rep, l = literal: the paths below put every one of the 12 states in front of a literal and in front of a match-type symbol"""
    c = to(hist(), 8)
    d = 4000
    for path in ("MlllM", "RlllR", "SlllS", "MMlM", "MQlR", "MlM", "MllM", "RlM", "RllM", "SlM", "SllM", "MMM", "RM", "SM", "MQM", "lll"):
        for k, ch in enumerate(path):
            if ch == "l":
                c.lit(rnd(1, c.here()))
            elif ch == "M":
                d += 1
                c.match(5, d)
            elif ch == "Q":                                          # rep0 directly behind its match: only a cut makes one -- the 27 bytes behind 273
                c.match(295, d)
            elif ch == "R":
                c.match(5, d)
            else:
                c.match(1, d)
        c.lit(rnd(4, c.here()))
    st, sym = check(T, O, "states", c.end_block())
    lit = {q.state for q in sym.values() if q.kind in (LIT, MLIT)}
    mat = {q.state for q in sym.values() if q.kind not in (LIT, MLIT)}
    assert lit == set(range(12)) and mat == set(range(12)), (sorted(lit), sorted(mat))


def test_matched_literals_agreeing_in_0_to_8_leading_bits(T, O):
    c = to(hist(), 8)
    for k in range(9):                                               # the byte behind the match agrees with the byte at the match distance in exactly k leading bits
        want = R[BLOCK - 5000 + c.here() + 6]                        # what a match of distance 5000 would copy next
        lit = want if k == 8 else want ^ (0x80 >> k)
        c.match(6, 5000).lit(bytes([lit])).lit(rnd(3, k))
    st, sym = check(T, O, "matched_literals", c.end_block())
    x = c.x()
    ml = [q for q in sym.values() if q.kind == MLIT]
    agree = []
    for q in ml:
        a, b = x[q.pos], x[q.pos - q.dist]
        agree.append(8 if a == b else 8 - int(a ^ b).bit_length())
    assert sorted(agree) == list(range(9)), agree


@pytest.mark.parametrize("rep", [False, True])
def test_lengths_at_every_position_state(T, O, rep):
    c = to(hist(), 8)
    want = []
    for ps in range(4):
        for ml in (2, 3, 4, 9, 10, 17, 18, 273):
            c.lit(rnd(4 + (ps - c.here()) % 4, c.here()))           # >= 4 literals, up to the position state
            if c.here() % RC + ml + 4 >= RC:
                to(c, (c.here() // RC + 1) * RC + 4 + ps)
            if rep:
                c.match(3, 7000).lit(rnd(4, c.here() + 1))
            want.append((c.here() & 3, ml))
            c.match(ml, 7000 if rep else 7000 + len(want))
    st, sym = check(T, O, "lengths_%d" % rep, c.lit(rnd(3, 1)).end_block())
    kind = REP0 if rep else MATCH
    got = {(q.pos & 3, q.length) for q in sym.values() if q.kind == kind}
    assert {(ps, ml) for ps in range(4) for ml in (2, 9, 10, 17, 18, 273)} <= got
    if not rep:
        assert {min(q.length - 2, 3) for q in sym.values() if q.kind == MATCH} == {0, 1, 2, 3}                        # the four length states of the slot coder


def test_first_and_last_distance_of_every_slot(T, O):
    """three blocks: two of history, then every slot's first and last distance up to the largest that 256 KiB + the block reach (slot 35: 196 609 .. 262 144)"""
    c = P.Composer().lit(R).end_block(full=True).lit(rnd(BLOCK, 31)).end_block(full=True)
    c.lit(rnd(8, 1))
    dists = []
    for slot in range(36):
        if slot < 4:
            lo = hi = slot
        else:
            nb = (slot >> 1) - 1
            lo = (2 | (slot & 1)) << nb
            hi = lo + (1 << nb) - 1
        dists += [lo + 1, hi + 1]
    dists = sorted(set(dists))
    assert dists[-1] == 2 * BLOCK
    for d in dists:
        c.match(3, d).lit(rnd(2, d))
    c.end_block()
    st, sym = check(T, O, "slots", c, win_cost=costs(c, [HOPELESS, HOPELESS, CHEAP]), stored={0, 1})
    got = sorted({q.dist for q in sym.values() if q.kind == MATCH} | {q.dist for q in sym.values() if q.kind in (REP0, REP1, REP2, REP3)})
    assert got == dists


# ---------------------------------------------------------------------------------------------- the entry refuses what the kernels were not sized for
def test_entry_refuses_bad_parses(T, pkg, monkeypatch):
    x = np.frombuffer(R[:1000], dtype=np.uint8)
    rec = lambda *rows: np.array(rows, dtype=np.uint32).reshape(-1, 2)
    bad = {"more records than a block's workspace holds": (0, rec(*[(0, (1 << 8) | 1)] * (MAX_SEQ + 1))),
           "more literals than the block is long": (1001, rec()),
           "litRank decreases or exceeds nLit": (990, rec((991, (5 << 8) | 10))),
           "litRank decreases or exceeds nLit ": (980, rec((500, (5 << 8) | 10), (499, (5 << 8) | 10))),
           "a record of length 0": (1000, rec((500, 5 << 8))),
           "an offset of 0": (990, rec((500, 10))),
           "an offset that reaches in front of the input": (990, rec((500, (501 << 8) | 10))),
           "literals and matches do not add up to the block's length": (900, rec((500, (5 << 8) | 10))),
           "literals and matches do not add up to the block's length ": (995, rec((500, (5 << 8) | 10)))}
    for what, blk in bad.items():
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM.*" + what.strip()):
            T.encode(x, [blk])
    for good in ((990, rec((500, (500 << 8) | 10))), (998, rec((500, (5 << 8) | 1), (998, (5 << 8) | 1)))):      # the largest offset that is inside; records of one byte
        assert len(I.inspect(T.encode(x, [good])).content) == 1000
    monkeypatch.setenv("GC_FRAME_BLOCKS", "1")                       # frames of one block: a match of block 1 may not reach into block 0
    small = Runner(pkg, T.name, T.kw)
    x2 = np.frombuffer(R + R[:100], dtype=np.uint8)
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM.*in front of its frame"):
        small.encode(x2, [(BLOCK, rec()), (90, rec((50, (51 << 8) | 10)))])
    small.close()
    shipped = pkg.load_library() if os.path.exists(pkg.LIB_PATH) else None
    for entry in ("gc_test_flzma2_encode_parsed", "gc_test_lzma2_rc_words"):
        assert getattr(shipped, entry, None) is None, "the shipped library exports the test entry"


# ---------------------------------------------------------------------------------------------- L3 on words
W_BIT, W_DIRECT = 0x0800, 0x4000
STRIDE = RC + 1024


def rc_reference(words):
    """the classical range encoder (cache + pending count) over (probability, bit) words -> its bytes"""
    low, rng, cache, pending, out = 0, 0xFFFFFFFF, 0, 1, bytearray()
    def shift():
        nonlocal low, cache, pending
        if low < 0xFF000000 or low >= (1 << 32):
            carry, t = low >> 32, cache
            while pending:
                out.append((t + carry) & 0xFF)
                t = 0xFF
                pending -= 1
            cache = (low >> 24) & 0xFF
        pending += 1
        low = (low & 0x00FFFFFF) << 8
    for w in words:
        w = int(w)
        bit = 1 if w & W_BIT else 0
        if w & W_DIRECT:
            rng >>= 1
            if bit:
                low += rng
        else:
            bound = (rng >> 11) * (w & 0x7FF)
            if bit:
                low += bound
                rng -= bound
            else:
                rng = bound
        while rng < (1 << 24):
            rng = (rng << 8) & 0xFFFFFFFF
            shift()
    for _ in range(5):
        shift()
    return bytes(out)


def run_words(T, name, seqs, starts=None, seg_log=17, usize=None):
    """chunk k codes seqs[k], laid at word starts[k] of its segment's place (default: one behind the other) -> [(bytes or None, csize)]"""
    per_seg = 1 << (seg_log - 12)
    place = T.enc.stream_words(seg_log)
    n_rc = len(seqs)
    n_seg = -(-n_rc // 32) * (32 // per_seg)
    words = np.zeros(n_seg * place, np.uint16)
    chunks = np.zeros((n_rc, 4), np.uint32)
    at = 0
    for k, s in enumerate(seqs):
        if k % per_seg == 0:
            at = 0
        if s is None:
            continue
        a = starts[k] if starts is not None else at
        assert a >= at and a + len(s) <= place
        base = (k // per_seg) * place
        words[base + a:base + a + len(s)] = s
        chunks[k] = (RC if usize is None else usize[k], 0, a, a + len(s))
        at = a + len(s)
    out, cs = T.enc.rc_words(words, chunks, seg_log)
    same_as_emulator(T, name, out.tobytes() + cs.tobytes(), lambda emu: b"".join(v.tobytes() for v in emu.enc.rc_words(words, chunks, seg_log)))
    return [(None if cs[k] == 0xFFFFFFFF else out[k, :cs[k]].tobytes() if (usize is None or usize[k] <= RC) else out[k:].ravel()[:cs[k]].tobytes(), int(cs[k])) for k in range(n_rc)]


def random_words(g, n, probs):
    p = g.choice(np.array(probs), n) if len(probs) > 1 else np.full(n, probs[0])
    w = (p.astype(np.uint16) | (g.integers(0, 2, n).astype(np.uint16) << 11))
    direct = p == 0
    w[direct] = W_DIRECT | (w[direct] & W_BIT)
    return w.astype(np.uint16)


def test_words_every_length_at_every_alignment(T):
    g = np.random.default_rng(1)
    seqs, starts, at = [], [], 0
    for k in range(200):
        n, a = k // 8, k % 8
        if k % 32 == 0:
            at = 0
        at = (at + 7) // 8 * 8 + a + (8 if at % 8 > a else 0)
        at = at if at % 8 == a else (at // 8 + 1) * 8 + a
        seqs.append(random_words(g, n, [31, 300, 1024, 1900, 2017, 0]))
        starts.append(at)
        at += n
    got = run_words(T, "words_align", seqs, starts)
    for k, (b, cs) in enumerate(got):
        assert b == rc_reference(seqs[k]), "chunk %d: %d words at word %d" % (k, len(seqs[k]), starts[k])


@pytest.mark.parametrize("probs", [[31], [1024], [2017], [31, 200, 1024, 1800, 2017, 0], [0]], ids=["p31", "p1024", "p2017", "mixed", "direct"])
def test_words_random(T, probs):
    g = np.random.default_rng(2 + probs[0])
    seqs = [random_words(g, n, probs) for n in (1, 7, 64, 999, 5000, 6000)]
    if probs == [31]:                                                # the unlikely bit throughout: a shift step at almost every word
        seqs.append((np.full(3000, 31 | W_BIT)).astype(np.uint16))
    if probs == [2017]:
        seqs.append((np.full(3000, 2017)).astype(np.uint16))
    for k, (b, cs) in enumerate(run_words(T, "words_%d_%d" % (probs[0], len(probs)), seqs)):
        assert b == rc_reference(seqs[k]), "sequence %d" % k


def carry_chain(pre, greedy, carry, tail=0, kick=0xA5):
    """8 * pre direct 0 bits (shift steps with digit 0; the coder's state is the same behind any number of them), the eight direct bits `kick` -- behind their shift step
    low is 2^32 - 256 x kick and the interval reaches over 2^32: a carry can come from here on --, then `greedy` direct
    bits chosen so that low approaches 2^32 from below -- 1 while low + (range >> 1) < 2^32, else 0 -- then either the bit that pushes low over 2^32 (the carry runs through
    every 0xFF in front of it) or nothing, then `tail` adaptive 0 bits (they leave low alone)"""
    low, rng, out = 0, 0xFFFFFFFF, []
    def put(bit):
        nonlocal low, rng
        rng >>= 1
        if bit:
            low += rng
        out.append(W_DIRECT | (W_BIT if bit else 0))
        if rng < (1 << 24):
            low = (low & 0xFFFFFF) << 8
            rng = (rng << 8) & 0xFFFFFFFF
    for i in range(8 * pre):
        put(0)
    for i in range(8 if kick < 256 else 16):                         # (a kick of two bytes starts the greedy bits from another place: other run lengths)
        put((kick >> i) & 1)
    for _ in range(greedy):
        put(1 if low + (rng >> 1) < (1 << 32) else 0)
    if carry:
        for _ in range(64):                                          # go on until the rule says 0, and say 1 there
            if low + (rng >> 1) >= (1 << 32):
                put(1)
                break
            put(1)
        else:
            raise AssertionError("no carry to be had")
    return np.array(out + [1024] * tail, np.uint16)


def ff_run(b):
    """(start, length) of the longest run of 0xFF"""
    best, at = (0, 0), 0
    while at < len(b):
        if b[at] != 0xFF:
            at += 1
            continue
        e = at
        while e < len(b) and b[e] == 0xFF:
            e += 1
        if e - at > best[1]:
            best = (at, e - at)
        at = e
    return best


@pytest.mark.parametrize("run", [1, 63, 64, 65, 200])
def test_words_carry_chains(T, run):
    """a run of `run` 0xFF bytes that a carry does or does not run through, in three layouts: the run ends inside the flush bytes (nothing behind the chain); the same with
    as many shift steps in front as put its end on a 64-byte tile boundary of L3b; and with words behind it, so that the run lies among the shift steps' digits"""
    # the greedy rule lengthens the run by three bytes every 24 bits; which lengths it passes through depends on where it starts, i.e. on the kick
    found = None
    for kick in list(range(1, 256)) + [(b << 8) | a for a in (1, 0x80, 0xFF) for b in (0, 1, 0x7F, 0x80, 0xFF)]:
        for g0 in range(0, 49):
            n0 = ff_run(rc_reference(carry_chain(1, g0, False, 0, kick)))[1]
            if n0 > run or (run - n0) % 3:
                continue
            greedy = g0 + 8 * (run - n0)
            plain = rc_reference(carry_chain(1, greedy, False, 0, kick))
            s, n = ff_run(plain)
            if n == run and len(plain) - 5 < s + n < len(plain):
                found = (kick, greedy, s + n)
                break
        if found:
            break
    assert found, "no chain gives a run of %d" % run
    kick, greedy, end = found
    layouts = {"flush": (1, 0), "tile": (1 + (64 - end % 64) % 64, 0), "inside": (3, 300)}
    seqs, keys = [], []
    for key, (pre, tail) in sorted(layouts.items()):
        for carry in (False, True):
            seqs.append(carry_chain(pre, greedy, carry, tail, kick))
            keys.append((key, carry))
    got = run_words(T, "carry_%d" % run, seqs)
    for (key, carry), s, (b, cs) in zip(keys, seqs, got):
        ref = rc_reference(s)
        assert b == ref, "%s, carry %s" % (key, carry)
        pre, tail = layouts[key]
        plain = rc_reference(carry_chain(pre, greedy, False, 0, kick))
        st, n = ff_run(plain)
        assert n == run and (key != "tile" or (st + n) % 64 == 0)
        if carry:                                                    # the carry came: the byte in front of the run is one more, the run's digits (all but the flush bytes) are 0x00
            assert ref[st - 1] == plain[st - 1] + 1 and ref[st:st + max(0, n - 4)] == b"\x00" * max(0, n - 4)
        elif not tail:
            assert ref == plain


def test_words_chunk_outgrows_staging(T):
    g = np.random.default_rng(9)
    big = random_words(g, 8 * (STRIDE + 40), [0])                    # 8 direct bits a byte: STRIDE + 40 bytes
    fits = random_words(g, 8 * (STRIDE - 40), [0])
    small = random_words(g, 100, [1024])
    got = run_words(T, "staging", [big, fits, small])
    assert got[0] == (None, 0xFFFFFFFF)
    assert got[1][0] == rc_reference(fits) and STRIDE - 40 <= got[1][1] <= STRIDE
    assert got[2][0] == rc_reference(small)


def test_words_group_above_64k_coded(T):
    g = np.random.default_rng(10)
    big = random_words(g, 8 * 65540, [0])                            # a group of 32 members has 160 KiB of staging, but an LZMA2 chunk holds 64 KiB coded
    ok = random_words(g, 8 * 65000, [0])
    seqs = [big] + [None] * 31 + [ok] + [None] * 31
    got = run_words(T, "group64k", seqs, usize=[BLOCK] + [0] * 31 + [BLOCK] + [0] * 31)
    assert got[0] == (None, 0xFFFFFFFF)
    assert got[32][1] <= 65536 and got[32][0] == rc_reference(ok)


def test_words_several_chunks_mixed_offsets(T):
    g = np.random.default_rng(11)
    seqs = [random_words(g, n, [31, 1024, 2017, 0]) for n in (300, 0, 4001, 17, 2500, 1, 64, 63, 65, 800)]
    starts = [3, 400, 401, 5000, 5100, 9000, 9001, 9100, 9200, 9300]
    for seg_log in (14, 17):
        got = run_words(T, "mixed_%d" % seg_log, seqs, starts if seg_log == 17 else None, seg_log=seg_log)
        for k, (b, cs) in enumerate(got):
            assert b == rc_reference(seqs[k]), "segLog %d chunk %d" % (seg_log, k)


def test_words_entry_refuses(T, pkg):
    place = T.enc.stream_words(17)
    words = np.full(place, 1024, np.uint16)
    ci = lambda *rows: np.array(rows, dtype=np.uint32).reshape(-1, 4)
    bad = {"segLog outside": (words, ci((RC, 0, 0, 10)), 13),
           "do not cover the places": (words[:-1], ci((RC, 0, 0, 10)), 17),
           "its word range leaves its segment's place": (words, ci((RC, 0, 0, place + 1)), 17),
           "its word range leaves its segment's place or overlaps": (words, ci((RC, 0, 0, 10), (RC, 0, 9, 20)), 17),
           "its members leave its segment": (words, ci((BLOCK, 0, 0, 10), (0, 0, 0, 0)), 17),
           "a member behind the leader is not absent": (words, ci((2 * RC, 0, 0, 10), (RC, 0, 10, 20)), 17)}
    for p in (30, 2018, 0):
        w = words.copy()
        w[5] = p
        bad["probability outside 31..2017 (%d)" % p] = (w, ci((RC, 0, 0, 10)), 17)
    for what, (w, c, seg_log) in bad.items():
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM.*" + what.split(" (")[0]):
            T.enc.rc_words(w, c, seg_log)
    w = words.copy()
    w[5], w[6], w[12] = 31, 2017, 7                                  # the edges are accepted; word 12 lies outside every chunk
    out, cs = T.enc.rc_words(w, ci((RC, 0, 0, 10)), 17)
    assert out[0, :cs[0]].tobytes() == rc_reference(w[:10])
