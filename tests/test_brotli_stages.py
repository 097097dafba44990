"""The brotli encoder's block stage -- B1 (gc_brotli_block_kernel), plan and emit (gc_brotli.hip) and the launches they share with the stream call (gc_api.hip
brotli_code_blocks) -- on EXACT parses, one named case per branch.  The test entry gc_test_brotli_encode_parsed (test builds only) takes the literals and records the match
finder would have left, so a case decides what B1 gets; tests/brotli_parse.py composes the blocks, derives the records and holds the models of the decoder's distance ring
and of the substitution pass; tests/brotli_inspect.py (a reader written from RFC 7932) says what the encoder wrote.  Every case asserts

    (a) the inspector's content is the input; this project's BrotliDecoder gives the input; so does the reference's decoder (where oracle/_ref is built), on the brotli-mt
        stream and on every frame's payload,
    (b) the commands the inspector reads are exactly the parse that went in -- insert length, copy length, resolved distance, chains merged -- and the distance symbol is
        the one DESIGN.md documents (0 substitution passes unless the case is about substitution; those compare with the model of the pass),
    (c) the inspector shows the branch the case is named after,
    (d) on the device: the bytes are the emulator's,
and of every prefix code of every compressed meta-block: a complete Kraft sum (the inspector refuses anything else), depths of at most 15 (5 for the code-length code), the
cost of an unbounded Huffman code for the same counts where that stays within the limit, otherwise no more than a fixed-length code over the used symbols.

A case is one chunk of two blocks as a rule: 128 KiB of random bytes (which B1 must store; the history the copies reach into), then the block under test, short and last.

What B1 decides differently from what one might expect, asserted as it decides it:
  * command 0 of a meta-block never uses the ring: its distance is explicit even where it equals the previous meta-block's last one (`ring_previous_meta_block`).
  * a code of 2 .. 4 symbols is written as a complex code, never as a simple one; the simple form appears for 0 and 1 symbols only.
  * the stored fallback needs `bits + 64 >= 8 * length`: with a stream header the shortest block that stays compressed has 18 bytes (`shortest_compressed`).
  * `GC_MAX_SEQ_PER_BLOCK` commands AND a tail: the block is stored (no entry of the row is left for the tail's command; `commands_row_full_with_tail`).
The 63-bit worst case -- an insert >= 22594 in front of a copy >= 2118 under a 15-bit command code -- is reached (`worst_case_63_bits`: Fibonacci counts
over 16 command symbols give the rarest one 15 bits without the limiter).

The geometric sweep of `test_limiter_sweep` (literals, 100 000 of them, counts ~ ratio^-k over n symbols, at least 1 each; the path is the one the test's model of
DESIGN.md's limiter takes, and the depths the inspector reads are that model's; bits over the package-merge optimum in brackets, printed, not asserted):
    no limiter (depth <= 15)            ratio 1.2 at 16, 32; 1.4 at 16; 1.6 at 16, 32, 64, 128; 2.0 at 16
    clamp, debt repaid exactly          1.2 at 64 (3); 1.4 at 32 (2), 64 (66); 2.0 at 32 (5)
    overshoot repair (debt < 0)         1.2 at 128 (46), 256 (265); 1.4 at 128 (181), 256 (732); 1.6 at 256 (12); 2.0 at 64 (112), 128 (201), 256 (380)
    give-up (debt != 0 -> stored)       none: see "Unreachable"
Fibonacci counts over 24 literal values (23 deep unbounded): overshoot repair, 390 bits over the optimum of 317 791.

Unreachable (each with its argument):
  * the limiter's give-up.  The debt after the clamp is repaid from depth 14 down, least frequent symbols first, in steps that halve from depth to depth, so it reaches 0
    or overshoots by less than one step of the depth it stops in; the repair then needs that many symbols at 15 bits, and a clamped code has them in every histogram that
    `test_limiter_never_gives_up` tries on the model (geometric ratios 1.05 .. 3 over 17 .. 704 symbols, heavy-tailed random counts, Fibonacci counts over 17 .. 24): none
    reaches `debt != 0`.  No proof that none can.
  * the lone code-length symbol in the command and distance alphabets.  It needs the used symbols to be exactly 0 .. 2^d - 1 at one depth.  Command 0 of a meta-block is in
    an explicit cell (symbol >= 128) and its distance symbol is >= 16, so the sets would have to be all of 0 .. 255 / 0 .. 1023 (no power of two reaches 704) or 0 .. 63,
    and distance symbol 63 stands for distances above 16 MiB.  Literals reach it ({0, 1}, {0 .. 3}, all 256).
  * `last - 3` (codes 8 and 14) when the last distance is 3 or less: the distance would be 0 or negative, which no parse can state (the entry refuses offset 0).  The case
    `ring_small_last` has what remains: last = 3 and 2 with the codes that do exist.
  * distances above 1 MiB (cases hold nine blocks at most): distance symbols 54 .. 63."""
import heapq
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import brotli_build as B
import brotli_inspect as I
import brotli_parse as P

BLOCK = P.BLOCK_MAX
MAX_SEQ = P.MAX_SEQ
R = np.random.default_rng(20260).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()      # block 0 of most cases
PLAIN, NOT_FIRST, NOT_LAST = 1, 2, 4


# ---------------------------------------------------------------------------------------------- the two backends
class Runner:
    def __init__(self, pkg, name, kw):
        self.name, self.pkg, self.kw = name, pkg, kw
        self.enc, self.dec = pkg.BrotliEncoder(level=6, **kw), pkg.BrotliDecoder(**kw)
        if name == "gpu":
            import torch
            self.torch = torch

    def encode(self, x, blocks, level=6, **kw):
        self.enc.set_level(level)
        cap = self.enc.compress_bound(x.size)
        if self.name == "gpu":
            t = self.torch
            d_src, d_dst = t.from_numpy(np.array(x)).to("cuda:0"), t.full((cap,), 0xA5, dtype=t.uint8, device="cuda:0")
            t.cuda.synchronize()
            self.enc.code_parsed_device(d_src.data_ptr(), x.size, d_dst.data_ptr(), cap, blocks, **kw)
            return d_dst[:self.enc.finish()].cpu().numpy().tobytes()
        src, dst = np.ascontiguousarray(x), np.full(cap, 0xA5, np.uint8)
        self.enc.code_parsed_device(src.ctypes.data, x.size, dst.ctypes.data, cap, blocks, **kw)
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


# ---------------------------------------------------------------------------------------------- prefix codes: what can be derived
def huffman_depths(counts):
    """the code lengths of an (unbounded) Huffman code for {symbol: count}.  Among equal weights a leaf goes before a merged node, leaves in symbol order, merged nodes in the
    order they were made (leaves sorted by (count, symbol), two-queue merge)"""
    syms = sorted(counts)
    heap = [(counts[s], 0, i) for i, s in enumerate(syms)]
    heapq.heapify(heap)
    parent, made = {}, 0
    while len(heap) > 1:
        n1, k1, i1 = heapq.heappop(heap)
        n2, k2, i2 = heapq.heappop(heap)
        parent[(k1, i1)] = parent[(k2, i2)] = (1, made)
        heapq.heappush(heap, (n1 + n2, 1, made))
        made += 1
    depth_of = {(1, made - 1): 0}
    for node in range(made - 2, -1, -1):
        depth_of[(1, node)] = depth_of[parent[(1, node)]] + 1
    return {s: (depth_of[parent[(0, i)]] + 1 if made else 0) for i, s in enumerate(syms)}


def limited_depths(counts, limit=15):
    """DESIGN.md "Length limit": clamp at `limit`; debt = Kraft sum - 1 in units of 2^-limit; from depth limit - 1 down to 1, symbols in ascending (count, symbol) order: a
    symbol of that depth goes one deeper while debt > 0; then, most frequent first, symbols at `limit` come up one while debt < 0.  -> (depths or None for the give-up, path)"""
    d = huffman_depths(counts)
    if max(d.values()) <= limit:
        return d, "none"
    order = sorted(counts, key=lambda s: (counts[s], s))
    for s in order:
        d[s] = min(d[s], limit)
    debt = sum(1 << (limit - d[s]) for s in order) - (1 << limit)
    for bl in range(limit - 1, 0, -1):
        for s in order:
            if debt > 0 and d[s] == bl:
                d[s] = bl + 1
                debt -= 1 << (limit - 1 - bl)
    path = "exact" if debt == 0 else "repair"
    for s in reversed(order):
        if debt < 0 and d[s] == limit:
            d[s] = limit - 1
            debt += 1
    return (d, path) if debt == 0 else (None, "give-up")


def package_merge_cost(counts, limit):
    """the cost of an optimal code with depths <= limit (package-merge)"""
    leaves = sorted((n, (s,)) for s, n in counts.items())
    if len(leaves) < 2:
        return 0
    packages = list(leaves)
    for _ in range(limit - 1):
        paired = [(packages[i][0] + packages[i + 1][0], packages[i][1] + packages[i + 1][1]) for i in range(0, len(packages) - 1, 2)]
        packages = sorted(leaves + paired, key=lambda p: p[0])
    depth = {s: 0 for s in counts}
    for _, members in packages[:2 * len(leaves) - 2]:
        for s in members:
            depth[s] += 1
    assert sum(2.0 ** -v for v in depth.values()) <= 1.0 + 1e-12
    return sum(counts[s] * depth[s] for s in counts)


def check_code(what, code, counts, limit=15):
    """a code against the counts of the symbols coded with it"""
    used = {s: n for s, n in counts.items() if n}
    if len(used) <= 1:
        assert code.kind == "simple" and code.nsym == 1 and code.single == (next(iter(used)) if used else 0), "%s: %d symbols are not the simple code of one" % (what, len(used))
        return
    assert code.kind == "complex", "%s: %d symbols under a simple code" % (what, len(used))
    assert {s for s, d in enumerate(code.depths) if d} == set(used), "%s: the code's symbols are not the used ones" % what
    assert max(code.depths) <= limit, "%s: depth %d" % (what, max(code.depths))
    free = huffman_depths(used)
    cost, total = code.cost(used), sum(used.values())
    if max(free.values()) <= limit:
        assert cost == sum(used[s] * free[s] for s in used), "%s: %d bits, a Huffman code has %d" % (what, cost, sum(used[s] * free[s] for s in used))
    else:
        assert cost <= total * (len(used) - 1).bit_length(), "%s: %d bits, a fixed-length code has %d" % (what, cost, total * (len(used) - 1).bit_length())
    if limit == 15:                                                    # its description: the code-length code
        hist = {}
        for s, _ in code.cl_symbols:
            hist[s] = hist.get(s, 0) + 1
        assert 16 not in hist, "%s: a repeat of a non-zero length (B1 writes none)" % what
        assert code.skip == (0 if code.clc_lengths[1] or code.clc_lengths[2] else (2 if code.clc_lengths[3] else 3)), "%s: HSKIP %d" % (what, code.skip)
        if len(hist) == 1:
            assert code.clc.single == next(iter(hist)) and code.clc_stored + code.skip == 18
        else:
            clc = I.Code(); clc.depths = list(code.clc_lengths); clc.kind = "complex"
            assert {s for s, d in enumerate(code.clc_lengths) if d} == set(hist), what
            assert max(code.clc_lengths) <= 5
            free = huffman_depths(hist)
            if max(free.values()) <= 5:
                assert clc.cost(hist) == sum(hist[s] * free[s] for s in hist), "%s: the code-length code is not a Huffman code" % what
            else:
                assert clc.cost(hist) <= sum(hist.values()) * (len(hist) - 1).bit_length(), what
            assert code.clc_lengths[B.CLC_ORDER[code.skip + code.clc_stored - 1]] != 0, "%s: the code-length code lengths end with a zero" % what


def zero_run_symbols(depths):
    """DESIGN.md "Code descriptions": the depths up to the last used symbol; a run of 3 or more zeros leaves as symbol 17 with up to 10 zeros (3 extra bits), and where zeros
    still follow, a plain 0 comes next, so two 17s never stand side by side -> [(symbol, extra)]"""
    last = max(s for s, d in enumerate(depths) if d)
    out, i = [], 0
    while i <= last:
        if depths[i]:
            out.append((depths[i], 0))
            i += 1
            continue
        run = 0
        while depths[i + run] == 0:
            run += 1
        if run >= 3:
            r = min(run, 10)
            out.append((17, r - 3))
            i += r
            if depths[i] == 0:
                out.append((0, 0))
                i += 1
        else:
            out.append((0, 0))
            i += 1
    return out


def meta_block_counts(mb):
    """what was coded with each code of a compressed meta-block: ([literal counts per tree], command counts, distance counts)"""
    lit = [dict() for _ in range(mb.ntreesl)]
    cmd, dist, at = {}, {}, 0
    for c in mb.commands:
        cmd[c.symbol] = cmd.get(c.symbol, 0) + 1
        for t, byte in zip(c.trees, mb.content[at:at + c.insert]):
            lit[t][byte] = lit[t].get(byte, 0) + 1
        at += c.insert + (0 if c.ended else c.copy)
        if isinstance(c.dsym, int):
            dist[c.dsym] = dist.get(c.dsym, 0) + 1
    return lit, cmd, dist


# ---------------------------------------------------------------------------------------------- assertions (a), (b), (d) and the codes
def check(T, O, name, comp, level=6, plain=0, rep_sub=0, ctx=False, stored=None):
    """-> the inspector's meta-block of every input block (and the stream's bytes as .stream of the first)"""
    x = comp.x()
    blocks = P.rows(x, comp.blocks)
    kw = dict(level=level, plain=plain, rep_sub=rep_sub, ctx_model=ctx)
    s = T.encode(x, blocks, **kw)
    if T.name == "emu":
        _EMU_BYTES[name] = s
    else:
        if name not in _EMU_BYTES:
            _EMU_BYTES[name] = T.emu.encode(x, blocks, **kw)
        assert s == _EMU_BYTES[name], "%s: the device's bytes differ from the emulator's" % name                     # (d)
    a = np.frombuffer(s, dtype=np.uint8)
    stored = getattr(comp, "stored", set()) if stored is None else set(stored)
    if plain:
        return s, x, blocks                                            # (pieces: the caller joins them)
    assert np.array_equal(T.dec.code(a), x), "%s: this project's decoder" % name                                     # (a)
    ref = O.ref("brotli") is not None
    if ref:
        assert np.array_equal(O.ref_brotlimt_decompress(a, x.size), x), "%s: the reference's brotli-mt decoder" % name
    frames = I.frames(s)
    bpc = 8 * level
    assert len(frames) == (len(comp.blocks) + bpc - 1) // bpc
    out, at = [], 0
    for f, (csize, hint, payload) in enumerate(frames):
        mine = comp.blocks[f * bpc:(f + 1) * bpc]
        size = sum(n for _, n, _ in mine)
        assert hint == (size >> 16) + 1, "%s: frame %d hint %d" % (name, f, hint)
        st = I.inspect(payload)
        assert st.wbits == 24 and st.size == len(payload) and st.content == x[at:at + size].tobytes(), "%s: frame %d" % (name, f)
        if ref:
            assert np.array_equal(O.ref_brotli_decompress(np.frombuffer(payload, np.uint8), size), x[at:at + size]), "%s: the reference's decoder on frame %d" % (name, f)
        out += match_blocks(name, st, x, mine, [f * bpc + i in stored for i in range(len(mine))], rep_sub, P.Ring(), last=True)
        at += size
    out[0].stream = s
    return out


def match_blocks(name, st, x, mine, is_stored, rep_sub, ring, last, first=True):
    """the meta-blocks of one stream against the input blocks it holds: kinds, (b), codes -> the meta-block of every input block"""
    kinds = [k for stored in is_stored for k in (("stored",) if stored else ("compressed", "metadata"))] + (["empty last"] if last else [])
    assert [mb.kind for mb in st.blocks] == kinds, "%s: meta-blocks %r, expected %r" % (name, [mb.kind for mb in st.blocks], kinds)
    out, k = [], 0
    for (start, n, seqs), stored in zip(mine, is_stored):
        mb = st.blocks[k]
        k += 1 if stored else 2
        out.append(mb)
        assert mb.mlen == n and mb.nibbles == (4 if n <= 65536 else 5) and not mb.last, "%s: MLEN %d in %d nibbles" % (name, mb.mlen, mb.nibbles)
        assert mb.bit % 8 == (4 if mb is st.blocks[0] and first else 0), "%s: a meta-block that does not start on a byte" % name
        if stored:
            continue
        assert st.blocks[k - 1].mlen == 0 and st.blocks[k - 1].skipped == b"" and st.blocks[k - 1].end_bit % 8 == 0
        assert mb.nbltypes == (1, 1, 1) and mb.npostfix == 0 and mb.ndirect == 0 and mb.ntreesd == 1 and mb.ntreesl in (1, 13)
        want = P.expected(P.substitute(x, start, P.merged(seqs, n), rep_sub), ring)                                   # (b)
        got = [(c.insert, 0, 0, None) if c.ended else (c.insert, c.copy, c.distance, c.dsym) for c in mb.commands]
        assert len(got) == len(want), "%s: %d commands, the parse has %d" % (name, len(got), len(want))
        if got != want:
            j = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError("%s: command %d is %r, the parse says %r" % (name, j, got[j], want[j]))
        lit, cmd, dist = meta_block_counts(mb)
        for t in range(mb.ntreesl):
            check_code("%s: literal tree %d" % (name, t), mb.lit_codes[t], lit[t])
        check_code("%s: commands" % name, mb.cmd_codes[0], cmd)
        check_code("%s: distances" % name, mb.dist_codes[0], dist)
        for what, code in [("literal tree %d" % t, c) for t, c in enumerate(mb.lit_codes)] + [("commands", mb.cmd_codes[0]), ("distances", mb.dist_codes[0])]:
            if code.kind == "complex":
                assert code.cl_symbols == zero_run_symbols(code.depths), "%s: the code-length symbols of %s" % (name, what)
        if mb.ntreesl == 13:
            assert mb.modes == [B.UTF8] and mb.lit_map.rlemax == 0 and mb.lit_map.imtf == 0 and len(mb.lit_map.symbols) == 64
            cm = {}
            for v in mb.lit_map.map:
                cm[v] = cm.get(v, 0) + 1
            check_code("%s: context map" % name, mb.lit_map.code, cm)
    return out


def low(n, seed, k=16, first=97):
    """n literal bytes of k values (compressible: log2 k bits each)"""
    return (np.random.default_rng(seed).integers(0, k, n) + first).astype(np.uint8).tobytes()


def shuffled(counts, seed):
    """bytes with exactly this histogram ({symbol: count}), in an order that a seed fixes"""
    a = np.repeat(np.array(list(counts.keys()), dtype=np.uint8), list(counts.values()))
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def base(pad=1000):
    """block 0: the random block.  pad: so many literals of four values open block 1 (they belong to its first command), so that a block of a few commands has something to
    gain and stays compressed"""
    c = P.Composer()
    c.stored = {0}
    c.lit(R).end_block(full=True)
    return c.lit(low(pad, 999, 4)) if pad else c


def alone():
    c = P.Composer()
    c.stored = set()
    return c


def cells(mb):
    return {c.symbol >> 6 for c in mb.commands}


# ---------------------------------------------------------------------------------------------- the entry refuses what B1 was not sized for
X1000 = np.frombuffer(R[:1000], dtype=np.uint8)
_rec = lambda *rows: np.array(rows, dtype=np.uint32).reshape(-1, 2)
REFUSED = {"nLit above the block": (np.zeros(1001, np.uint8), _rec()),
           "litRank above nLit": (X1000[:990], _rec((991, (5 << 8) | 10))),
           "litRank decreasing": (X1000[:980], _rec((500, (5 << 8) | 10), (499, (5 << 8) | 10))),
           "a copy of 1": (X1000[:999], _rec((500, (5 << 8) | 1))),
           "too few bytes": (X1000[:900], _rec((500, (5 << 8) | 10))),
           "too many bytes": (X1000[:995], _rec((500, (5 << 8) | 10))),
           "offset 0": (X1000[:990], _rec((500, 10))),
           "offset in front of the chunk": (X1000[:990], _rec((500, (501 << 8) | 10))),
           "more records than a row holds": (X1000[:0], _rec(*[(0, (1 << 8) | 2)] * (MAX_SEQ + 1)))}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_entry_refuses(T, pkg, what):
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM.*parsed block 0"):
        T.encode(X1000, [REFUSED[what]])


def test_entry_refuses_counts_without_data(pkg, emu_lib_path):
    """(the Python method always hands data over: the raw entry, on the emulator library -- the check runs on the host before anything is launched)"""
    import ctypes as C
    T = Runner(pkg, "emu", dict(lib_path=emu_lib_path))
    fn = T.enc._lib.gc_test_brotli_encode_parsed
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    dst, meta, rec = np.zeros(4096, np.uint8), np.array([[1, 990]], np.uint32), _rec((500, (5 << 8) | 10))
    lit = np.ascontiguousarray(X1000[:990])
    assert fn(T.enc._ctx, X1000.ctypes.data, 1000, dst.ctypes.data, 4096, 6, 0, 0, 0, None, rec.ctypes.data, meta.ctypes.data) == -5
    assert b"parsed block 0: counts without data" in T.enc._lib.gc_last_error_message(T.enc._ctx)
    assert fn(T.enc._ctx, X1000.ctypes.data, 1000, dst.ctypes.data, 4096, 6, 0, 0, 0, lit.ctypes.data, None, meta.ctypes.data) == -5
    T.close()


def test_entry_accepts_the_neighbours(T, pkg):
    good = {"the largest offset inside the chunk": (X1000[:990], _rec((500, (500 << 8) | 10))),
            "a copy of 2": (X1000[:998], _rec((500, (5 << 8) | 2))),
            "litRank equal to nLit": (X1000[:990], _rec((990, (5 << 8) | 10))),
            "as many records as a row holds": (X1000[:0], None)}
    for what, (lit, rec) in good.items():
        if rec is None:                                                # MAX_SEQ records of 2 bytes at offset 1 behind one literal: a block of one byte value
            x = np.full(1 + 2 * MAX_SEQ, 7, np.uint8)
            blk = (x[:1], _rec(*[(1, (1 << 8) | 2)] * MAX_SEQ))
        else:
            x = X1000.copy()
            r, offml = rec[0].tolist()
            at, ml, off = r, offml & 255, offml >> 8
            x = np.concatenate([lit[:at], lit[at - off:at - off + ml] if off >= ml else np.resize(lit[at - off:at], ml), lit[at:]])
            blk = (lit, rec)
        s = T.encode(x, [blk])
        assert I.inspect(I.frames(s)[0][2]).content == x.tobytes(), what
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
        T.encode(X1000, [(X1000[:990], _rec((500, (500 << 8) | 10)))], plain=2)                                      # a later piece that is not a plain stream
    plain = T.encode(X1000[:1000], [(X1000, _rec())], plain=PLAIN)
    assert I.inspect(plain).content == X1000.tobytes()


def test_the_shipped_library_has_no_parsed_entry(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pytest.skip("shipped library not built")
    assert getattr(pkg.load_library(), "gc_test_brotli_encode_parsed", None) is None, "the shipped library exports the test entry"


def test_entry_offsets_in_a_plain_piece_and_behind_a_chunk_boundary(T, pkg):
    """in front of the call's first byte (plain) / of the block's brotli-mt chunk (level 1: block 8 opens a chunk)"""
    c = alone()
    for _ in range(8):
        c.lit(low(BLOCK, 1)).end_block(full=True)
    c.lit(low(100, 2)).copy(10, 100).end_block()
    x = c.x()
    rows = P.rows(x, c.blocks)
    T.encode(x, rows, level=1)
    lit, rec = rows[8]
    over = _rec((100, (101 << 8) | 10))
    with pytest.raises(pkg.GpuCodecError, match="parsed block 8: an offset that reaches in front of the chunk"):
        T.encode(x, rows[:8] + [(lit, over)], level=1)
    T.encode(x, rows[:8] + [(lit, over)], level=2)                    # 16 blocks per chunk: inside
    T.encode(x, rows[:8] + [(lit, over)], level=1, plain=PLAIN)       # one stream: inside


# ---------------------------------------------------------------------------------------------- length classes, cells
def test_insert_lengths(T, O):
    """every insert length class at its base and at the last value of the class in front of it (22593, 22594 included)"""
    lens = sorted({v for b in B.INS_BASE for v in (b, b - 1) if v >= 0})
    c = base(0)
    for i, n in enumerate(lens):
        c.lit(low(n, 100 + i)).copy(4, 1000 + 37 * i)
    mb = check(T, O, "insert_lengths", c.end_block())[1]
    assert [q.insert for q in mb.commands] == lens and {B.command_fields(q.symbol)[0] for q in mb.commands} == set(range(24))


def test_insert_longest(T, O):
    """the longest insert in front of a copy: the block but two bytes; and a block of literals only (trailing insert, explicit cell, empty distance alphabet)"""
    c = base(0)
    mb = check(T, O, "insert_longest", c.lit(low(BLOCK - 2, 5)).copy(2, 777).end_block())[1]
    assert [(q.insert, q.copy) for q in mb.commands] == [(BLOCK - 2, 2)] and mb.commands[0].symbol >> 6 == 7
    c = base(0)
    mb = check(T, O, "literals_only", c.lit(low(BLOCK, 6)).end_block())[1]
    assert len(mb.commands) == 1 and mb.commands[0].ended and mb.commands[0].insert == BLOCK and mb.commands[0].symbol >> 6 == 7
    assert mb.dist_codes[0].kind == "simple" and mb.dist_codes[0].single == 0 and mb.cmd_codes[0].kind == "simple"


def test_copy_lengths(T, O):
    """every copy length class at its base and at the last value of the class in front of it (2, 2117, 2118 included)"""
    lens = sorted({v for b in B.COPY_BASE for v in (b, b - 1) if v >= 2})
    c = base()
    for i, n in enumerate(lens):
        c.lit(low(1, 200 + i)).copy(n, 5000 + 41 * i)
    mb = check(T, O, "copy_lengths", c.end_block())[1]
    assert [q.copy for q in mb.commands] == lens and {B.command_fields(q.symbol)[1] for q in mb.commands} == set(range(24))


def test_one_copy_fills_the_block(T, O):
    """a block of one copy only: 131072 bytes (a chain of 515 records), an empty literal alphabet, one command, one distance"""
    c = base(0)
    mb = check(T, O, "one_copy", c.copy(BLOCK, BLOCK).end_block(full=True))[1]
    assert [(q.insert, q.copy, q.distance) for q in mb.commands] == [(0, BLOCK, BLOCK)]
    assert [k.kind for k in (mb.lit_codes[0], mb.cmd_codes[0], mb.dist_codes[0])] == ["simple"] * 3 and mb.lit_codes[0].single == 0
    assert mb.end_bit - mb.bit == mb.header_bits + 24 + 16                                          # 24 copy extra bits, 16 distance extra bits, no bit for a symbol


def test_every_cell(T, O):
    """the nine explicit cells and the two implicit ones; `ic < 8 && cc < 16`: insert 9 / copy 69 are the last implicit ones, insert 10 or copy 70 at the
    previous distance go to an explicit cell with distance symbol 0"""
    c = base()
    d = 3000
    want = []
    for ins in (0, 3, 9, 10, 50, 129, 130, 500):
        for cp in (2, 9, 10, 69, 70, 200):
            for same in (False, True):
                if not same:
                    d += 50
                if ins == 0 and same:
                    continue                                           # (no literals and the distance in front: the records merge)
                c.lit(low(ins, ins + cp)).copy(cp, d)
                want.append("implied" if same and ins < 10 and cp < 70 else (0 if same else None))
    mb = check(T, O, "every_cell", c.lit(low(5, 1)).end_block())[1]
    assert cells(mb) == set(range(11))
    for q, w in zip(mb.commands, want):
        assert w is None or q.dsym == w, (q.insert, q.copy, q.dsym, w)
        assert (q.symbol < 128) == (w == "implied")


@pytest.mark.parametrize("tail,cell", [(1, 0), (9, 0), (10, 4), (129, 4), (130, 7), (30000, 7)])
def test_trailing_insert(T, O, tail, cell):
    """the trailing insert-only command: an implicit cell below 10 literals, an explicit one from 10 (no distance follows either)"""
    c = base().lit(low(20, 3)).copy(30, 999)
    mb = check(T, O, "trailing_insert_%d" % tail, c.lit(low(tail, 4)).end_block())[1]
    q = mb.commands[-1]
    assert q.ended and q.insert == tail and q.symbol >> 6 == cell and B.command_fields(q.symbol)[1] == 0


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f


def test_worst_case_63_bits(T, O):
    """an insert of 22594 + in front of a copy of 2118 + under a 15-bit command code: 15 + 24 + 24 bits in one word.  Sixteen command symbols with Fibonacci counts give
    the rarest one 15 bits without the limiter"""
    c = base(0)
    big = (22594 + 40000, 2118 + 20000)
    cmds = [big]
    shapes = [(i, cp) for i in (1, 2, 3) for cp in (2, 3, 4, 5, 6)]
    for (ins, cp), n in zip(shapes, _fib(16)[1:]):
        cmds += [(ins, cp)] * n
    order = np.random.default_rng(7).permutation(len(cmds))
    d = 2000
    for k in order:
        d += 7
        c.lit(low(cmds[k][0], int(k), 4)).copy(cmds[k][1], d)
    assert c.here() <= BLOCK
    mb = check(T, O, "worst_case_63_bits", c.end_block())[1]
    q = next(q for q in mb.commands if q.insert == big[0])
    assert q.copy == big[1] and mb.cmd_codes[0].depths[q.symbol] == 15 and max(mb.cmd_codes[0].depths) == 15 and mb.cmd_codes[0].nsym == 16


# ---------------------------------------------------------------------------------------------- distances
def test_distance_buckets(T, O):
    """off + 3 = 2^k, 2^k - 1, 3 * 2^(k-1) and 3 * 2^(k-1) - 1: both halves of every bucket at their first and last value, up to the largest k two blocks allow; distance 1;
    the largest distance inside the chunk"""
    c = base().lit(low(70000, 8))
    series = [[(1 << k) - 3 for k in range(2, 18)], [(1 << k) - 4 for k in range(3, 18)], [(3 << (k - 1)) - 3 for k in range(2, 18)], [(3 << (k - 1)) - 4 for k in range(2, 18)]]
    dist = [d for s in series for d in s if d >= 1] + [len(c.out) + 2 * 70]
    for i, d in enumerate(dist):
        c.lit(low(1, i))
        c.copy(2, d if i < len(dist) - 1 else len(c.out))
    mb = check(T, O, "distance_buckets", c.end_block())[1]
    assert [q.distance for q in mb.commands[:-1]] == dist[:-1] and mb.commands[-1].distance == BLOCK + 1000 + 70000 + 3 * (len(dist) - 1) + 1
    assert all(isinstance(q.dsym, int) and q.dsym >= 16 for q in mb.commands), "a case that was meant to be explicit throughout"
    assert mb.commands[0].distance == 1 and {q.dsym for q in mb.commands} >= set(range(16, 16 + 2 * 16))


def _ring_block(c, heads):
    for i, d in enumerate(heads):
        c.lit(low(1, i)).copy(3, d)
    return c


@pytest.mark.parametrize("code", range(1, 16))
def test_ring_code(T, O, code):
    """each short code in turn, behind four explicit heads 9000, 7000, 5000, 3000 (oldest first)"""
    ring = [3000, 5000, 7000, 9000]
    d = ring[code] if code < 4 else ring[(code - 4) // 6] + [-1, 1, -2, 2, -3, 3][(code - 4) % 6]
    c = _ring_block(base(), [9000, 7000, 5000, 3000, d, 11000])
    mb = check(T, O, "ring_code_%d" % code, c.end_block())[1]
    e = lambda v: B.distance_code_for(v, 0, 0)[0]
    assert [q.dsym for q in mb.commands] == [e(9000), e(7000), e(5000), e(3000), code, e(11000)]


def test_ring_preferences(T, O):
    """where several codes spell a distance: 1 before 5 (second last == last + 1), 2 before 4, 3 before 6, 7 before 10 (last + 2 == second last - 1), 4 .. 9 in their order"""
    c = base()
    _ring_block(c, [9000, 7000, 5001, 5000, 5001])                    # ring 5000 5001 7000 9000: 5001 is entry 1 and last + 1
    _ring_block(c, [20000, 6999, 8000, 7000, 6999])                   # ring 7000 8000 6999 20000: 6999 is entry 2 and last - 1
    _ring_block(c, [30000, 2998, 31000, 32000, 3000, 2998])           # ring 3000 32000 31000 2998: 2998 is entry 3 and last - 2
    _ring_block(c, [40000, 4003, 4000, 4002])                         # ring 4000 4003 40000: 4002 is last + 2 and second last - 1
    _ring_block(c, [50000, 2, 1])                                     # last - 1 (4) where last - 3 would be negative
    mb = check(T, O, "ring_preferences", c.end_block())[1]
    got = [q.dsym for q in mb.commands]
    assert (got[4], got[9], got[15], got[19], got[22]) == (1, 2, 3, 7, 4), got


@pytest.mark.parametrize("back", [23, 24, 25])
def test_ring_walk_limit(T, O, back):
    """a head `back` commands in front: 9000, then a run of back - 1 commands at 5000 (a literal between them keeps them apart), then 9000 again.  The walk covers 24
    commands: entry 1 is known when the run's first command is at most 23 back, i.e. the head in front of it 24"""
    c = base().lit(b"x").copy(3, 20000).lit(b"x").copy(3, 9000)
    for i in range(back - 1):
        c.lit(low(1, i)).copy(3, 5000)
    mb = check(T, O, "ring_walk_%d" % back, c.lit(b"y").copy(3, 9000).lit(b"z").copy(3, 5001).end_block())[1]
    assert mb.commands[-2].dsym == (1 if back <= 24 else B.distance_code_for(9000, 0, 0)[0])
    assert mb.commands[-1].dsym == 11                                  # second last + 1: entry 1 is one command back here
    assert [q.dsym for q in mb.commands[3:-2]] == ["implied"] * (back - 2)


def _compressible_full_block(c, last):
    """a full block of literals whose last commands leave `last` as the ring's newest entries (oldest first)"""
    n = BLOCK - 4 * len(last)
    c.lit(low(n, 77))
    for d in last:
        c.lit(b"q").copy(3, d)
    return c.end_block(full=True)


def test_ring_previous_meta_block(T, O):
    """entries the previous meta-block left: B1 must not name them.  Command 0 at the previous block's last distance is explicit (the decoder then holds it twice);
    command 1 at the distance under it is explicit too (B1 knows one entry), and from command 2 on the codes resolve against the ring as the decoder has it"""
    c = alone()
    _compressible_full_block(c, [800, 700, 600, 500])
    c.lit(low(1000, 5, 4)).copy(3, 500).lit(b"b").copy(3, 600).lit(b"c").copy(3, 500).lit(b"d").copy(3, 601).lit(b"e").copy(3, 700).lit(b"f").copy(3, 600).lit(b"g").copy(3, 703)
    mb = check(T, O, "ring_previous_meta_block", c.end_block())[1]
    e = lambda d: B.distance_code_for(d, 0, 0)[0]
    assert [q.dsym for q in mb.commands] == [e(500), e(600), 1, 11, e(700), 3, 15], [q.dsym for q in mb.commands]


def test_ring_small_last(T, O):
    """last distances of 3 and less: the codes that would give 0 or less do not exist; those that remain are used"""
    c = _ring_block(base(), [3, 1, 3, 2, 5, 2, 1, 4, 1, 2, 3])
    mb = check(T, O, "ring_small_last", c.end_block())[1]
    assert [q.distance for q in mb.commands] == [3, 1, 3, 2, 5, 2, 1, 4, 1, 2, 3]
    assert [q.dsym for q in mb.commands] == [17, 6, 1, 4, 9, 1, 4, 9, 1, 3, 5], [q.dsym for q in mb.commands]


# ---------------------------------------------------------------------------------------------- substitution
PATTERN = np.random.default_rng(5).integers(0, 256, 64, dtype=np.uint8).tobytes()


class Periodic:
    """a block that continues one 64-byte pattern throughout: a copy at ANY multiple of 64 yields the same bytes, so every such distance is a candidate that matches"""
    def __init__(self, c, lead=1024):
        self.c, self.at = c, 0
        self.lit(lead)

    def lit(self, n):
        self.c.lit((PATTERN * (n // 64 + 2))[self.at % 64:self.at % 64 + n])
        self.at += n
        return self

    def copy(self, ml, d, ll=1):
        self.lit(ll)
        self.c.copy(ml, d)
        self.at += ml
        return self


def _sub_check(T, O, name, c, passes):
    x = c.x()
    start, n, seqs = c.blocks[-1]
    before = P.merged(seqs, n)
    after = P.substitute(x, start, before, passes)
    mb = check(T, O, "%s_%d" % (name, passes), c, rep_sub=passes)[-1]
    return mb, [a[2] for a in after], [b[2] for b in before]


@pytest.mark.parametrize("passes", [1, 2])
def test_substitution_candidates(T, O, passes):
    """a candidate one, two and three commands in front (the nearer ones copy from the random block and do not match); the break at a command of the copy's own distance
    hides a matching candidate behind it; copies of 512 bytes take part, of 513 do not"""
    p = Periodic(base(), 2048)
    far = lambda i: 100000 + 1000 * i                                  # into block 0: breaks the pattern for 4 bytes, which a literal run of the pattern then resumes
    def foreign(i):
        p.c.lit(b"!").copy(4, far(i))
        p.at += 5
        p.lit(3 + (64 - p.at % 64) % 64)                               # (the pattern's phase is kept: `at` counts every byte)
    p.copy(20, 64).copy(20, 128)                                                                    # k = 1
    p.copy(20, 64); foreign(1); p.lit(200).copy(20, 192)                                            # k = 2
    p.copy(20, 64); foreign(2); foreign(3); p.lit(200).copy(20, 256)                                # k = 3
    p.copy(20, 64).copy(20, 320); foreign(4); p.lit(200).copy(20, 320)                              # the break: 320, then a mismatch, then 320 again -- 64 is never looked at
    p.copy(600, 64).copy(512, 128).copy(600, 64).copy(513, 128)                                     # BR_SUB_MAX
    mb, after, before = _sub_check(T, O, "substitution_candidates", p.c.lit(b"end").end_block(), passes)
    assert after != before
    big = [(q.copy, q.distance) for q in mb.commands if q.copy >= 512]
    assert big == [(600, 64), (512, 64), (600, 64), (513, 128)]


@pytest.mark.parametrize("passes", [1, 2])
def test_substitution_at_the_end_of_the_input(T, O, passes):
    """a copy of fewer than 8 bytes that ends with the input (no 8-byte read across that end): one that matches at the candidate and one that differs in its last byte"""
    for kind in ("same", "differs"):
        c = base(0).lit(low(900, 1, 4))
        z = bytes(range(200, 207))
        z0 = c.here()
        c.lit(z + low(50, 1))
        z1 = c.here()
        c.lit((z if kind == "same" else z[:6] + b"\x00") + low(40, 2))
        at = c.here() + 6 + 1                                          # where the last copy will start
        c.lit(b"k").copy(5, at - z1)                                   # command 0: the distance that leads from there to the second z (any bytes here)
        c.lit(b"m").copy(7, at - z0)                                   # the last 7 bytes: z from its first occurrence
        mb, after, before = _sub_check(T, O, "substitution_end_%s" % kind, c.end_block(), passes)
        assert mb.commands[-1].copy == 7 and not mb.commands[-1].ended
        assert after[-1] == (before[-2] if kind == "same" else before[-1]), (kind, after, before)


@pytest.mark.parametrize("passes", [1, 2])
def test_substitution_tile_boundary(T, O, passes):
    """command 255 against command 256.  The same three copies -- 64, 128, 128, every multiple of 64 a candidate that matches -- stand at commands 99 / 100 / 101 (one tile)
    and at 254 / 255 / 256 (across the boundary).  The second takes 64 in both.  Inside a tile the third reads its predecessor's OLD 128, which is its own, and stays;
    across the boundary the predecessor's 64 is stored by then, and the third takes it.  The second pass tells them apart again: the first of the three took the 320 of
    the command in front of it in pass 1, the second takes that now; inside a tile the third reads the second's old 64 and takes it (128 -> 64), across the boundary it
    reads the 320 just stored (64 -> 320).  Two commands of tile 2
    depend on the copy lengths carried over from tile 1 (1606 bytes): a copy from the random block behind a command at 64, which matches at 64 only 1606 bytes further
    up, in the pattern -- taken with the carry lost, the content is wrong; and a copy of twenty bytes that stand 100 and 200 in front of it, stated at 200 behind a command at
    100, which takes the 100 where it stands and finds nothing with the carry lost"""
    p = Periodic(base(), 4096)

    def triple():
        p.copy(20, 64).copy(20, 128).copy(20, 128)

    n = 0
    while n < 254:
        if n == 99:
            triple(); n += 3
        else:
            p.copy(6, 64 * (2 + n % 5)); n += 1
    triple()
    c = p.c
    carried = sum(ml for _, ml, _ in c.seqs[:256])
    p.lit(200).copy(20, 64)                                            # command 257, at 64 ...
    c.lit(b"!").copy(20, c.here() + 50000)                             # ... and 258: twenty bytes of the random block
    z, w = bytes(range(100, 120)), np.random.default_rng(12).integers(0, 256, 160, dtype=np.uint8).tobytes()
    c.lit(z + w[:80] + z + w[80:154]).copy(5, 100).lit(b"?").copy(20, 200)        # 259 at 100 (any bytes), 260: z, which stands 200 and 100 in front of it
    assert len(c.seqs) == 261 and carried == 1606
    mb, after, before = _sub_check(T, O, "substitution_tile_boundary", c.lit(b"end").end_block(), passes)
    got = [q.distance for q in mb.commands]
    assert before[99:102] == before[254:257] == [64, 128, 128]
    inside, across = ([64, 128], [64, 64]) if passes == 1 else ([320, 64], [320, 320])
    assert after[100:102] == inside and got[100:102] == inside, (after[100:102], got[100:102])
    assert after[255:257] == across and got[255:257] == across, (after[255:257], got[255:257])
    assert before[258] == after[258] == got[258] > 50000 and before[257] == 64                          # the random block's bytes do not stand at 64
    assert (before[259:261], after[259:261], got[259:261]) == ([100, 200], [100, 100], [100, 100])


@pytest.mark.parametrize("passes", [1, 2])
def test_substitution_second_pass(T, O, passes):
    """a run of copies at 64, 128, 192 ... that all match at every multiple of 64: a pass moves each distance one command along (reads before stores), the second pass once more"""
    p = Periodic(base(), 2048)
    p.copy(20, 64)
    for i in range(8):
        p.copy(20, 64 * (i + 2))
    mb, after, before = _sub_check(T, O, "substitution_second_pass", p.c.lit(b"end").end_block(), passes)
    want = [64] * (1 + passes) + [64 * i for i in range(2, 10 - passes)]      # (every multiple of 64 matches: a pass hands each command its predecessor's distance)
    assert after[:9] == want and [q.distance for q in mb.commands[:9]] == want, after


# ---------------------------------------------------------------------------------------------- prefix codes
def _lit_block(c, lit, n_copies=4, copy_len=5):
    """the literals of a block cut around a few fixed copies into block 0"""
    n = len(lit)
    at = 0
    for k in range(n_copies):
        cut = (k + 1) * n // (n_copies + 1)
        c.lit(lit[at:cut]).copy(copy_len + 3 * k, 60000 + 999 * k)
        at = cut
    return c.lit(lit[at:]).end_block()


@pytest.mark.parametrize("values", [(65,), (65, 66), (0, 1), (0, 1, 2, 3), tuple(range(256))])
def test_literal_alphabets(T, O, values):
    """1 and 2 symbols; {0, 1}, {0 .. 3} and all 256 with equal counts: every depth the same and the symbols 0 .. 2^d - 1, so the description has ONE code-length symbol"""
    lit = shuffled({v: 4096 // len(values) for v in values}, 3)
    mb = check(T, O, "literal_alphabet_%d_%d" % (values[0], len(values)), _lit_block(base(0), lit, copy_len=2000 if len(values) == 256 else 5))[1]
    code = mb.lit_codes[0]
    if len(values) == 1:
        assert code.kind == "simple" and code.single == 65
    else:
        d = (len(values) - 1).bit_length()
        assert code.kind == "complex" and [code.depths[v] for v in values] == [d] * len(values)
        lone = values[0] == 0
        assert (code.clc.single == d) == lone and (not lone or (code.cl_symbols == [(d, 0)] * len(values) and code.clc_stored + code.skip == 18))
        assert code.skip == (3 if d == 8 else 0)                       # lengths 1 and 2 stand first in the eighteen; 8 stands behind 1, 2, 3 (and no other symbol is used)


def test_command_and_distance_alphabets(T, O):
    """1 and 2 symbols in the command and distance alphabets: one command (simple codes), two commands of two shapes, fifty equal commands (one explicit, the rest implied)"""
    mb = check(T, O, "alphabets_one_command", base().lit(low(40, 1)).copy(9, 4444).end_block())[1]
    assert mb.cmd_codes[0].kind == "simple" and mb.dist_codes[0].kind == "simple" and mb.dist_codes[0].single == B.distance_code_for(4444, 0, 0)[0]
    mb = check(T, O, "alphabets_two_commands", base().lit(low(40, 1)).copy(9, 4444).lit(low(3, 2)).copy(4, 17).end_block())[1]
    assert mb.cmd_codes[0].nsym == 2 and mb.dist_codes[0].nsym == 2 and mb.cmd_codes[0].kind == "complex" and max(mb.cmd_codes[0].depths) == 1
    c = base()
    for i in range(50):
        c.lit(low(2, i)).copy(4, 4444)
    mb = check(T, O, "alphabets_fifty_equal", c.end_block())[1]
    assert mb.cmd_codes[0].nsym == 2 and mb.dist_codes[0].kind == "simple" and [q.dsym for q in mb.commands[1:]] == ["implied"] * 49


LIMITER_EXCESS = {}


def test_fibonacci_literals(T, O):
    """Fibonacci counts over 24 literal values: an unbounded code would be 23 deep; the limiter clamps at 15"""
    counts = {40 + i: n for i, n in enumerate(_fib(24))}
    mb = check(T, O, "fibonacci_literals", _lit_block(base(0), shuffled(counts, 9)))[1]
    code = mb.lit_codes[0]
    assert max(code.depths) == 15 and max(huffman_depths(counts).values()) == 23
    model, path = limited_depths(counts)
    assert path != "none" and [code.depths[s] for s in sorted(counts)] == [model[s] for s in sorted(counts)]
    LIMITER_EXCESS["fibonacci_literals"] = code.cost(counts) - package_merge_cost(counts, 15)
    print("fibonacci_literals: path %s, %d bits over the length-limited optimum of %d" % (path, LIMITER_EXCESS["fibonacci_literals"], package_merge_cost(counts, 15)))


def test_fibonacci_commands(T, O):
    """Fibonacci counts over 18 command symbols (17 deep unbounded)"""
    shapes = [(i, cp) for i in (1, 2, 3) for cp in (2, 3, 4, 5, 6, 7)]
    cmds = [s for s, n in zip(shapes, _fib(18)) for _ in range(n)]
    c = base(0)
    d = 2000
    for k in np.random.default_rng(3).permutation(len(cmds)):
        d += 7
        c.lit(low(cmds[k][0], int(k), 4)).copy(cmds[k][1], d)
    mb = check(T, O, "fibonacci_commands", c.end_block())[1]
    code = mb.cmd_codes[0]
    _, cmd, _ = meta_block_counts(mb)
    assert code.nsym == 18 and max(code.depths) == 15 and max(huffman_depths(cmd).values()) == 17
    model, path = limited_depths(cmd)
    assert path != "none" and all(code.depths[s] == model[s] for s in cmd)
    LIMITER_EXCESS["fibonacci_commands"] = code.cost(cmd) - package_merge_cost(cmd, 15)
    print("fibonacci_commands: path %s, %d bits over the length-limited optimum" % (path, LIMITER_EXCESS["fibonacci_commands"]))


SWEEP = [(r, n) for r in (1.2, 1.4, 1.6, 2.0) for n in (16, 32, 64, 128, 256)]
SWEEP_PATH = {}


def _geometric(ratio, n, total=100000):
    w = np.array([ratio ** -k for k in range(n)])
    cnt = np.maximum(1, np.floor(w / w.sum() * total)).astype(int)
    return {s: int(k) for s, k in enumerate(cnt)}


@pytest.mark.parametrize("ratio,n", SWEEP)
def test_limiter_sweep(T, O, ratio, n):
    """which path of the limiter a geometric histogram takes (the test's model of DESIGN.md's text decides; the depths read back are the model's)"""
    counts = _geometric(ratio, n)
    model, path = limited_depths(counts)
    assert model is not None, "a histogram that reaches the give-up: move it to a case of its own"
    mb = check(T, O, "limiter_sweep_%s_%d" % (ratio, n), _lit_block(base(0), shuffled(counts, n)))[1]
    code = mb.lit_codes[0]
    assert [code.depths[s] for s in sorted(counts)] == [model[s] for s in sorted(counts)], path
    assert (max(code.depths) == 15) == (path != "none") or max(huffman_depths(counts).values()) == 15
    SWEEP_PATH[(ratio, n)] = path
    print("limiter sweep: ratio %s, %d symbols: %s, %d bits over the optimum" % (ratio, n, path, code.cost(counts) - package_merge_cost(counts, 15)))


def test_limiter_never_gives_up():
    """the argument of "Unreachable" on the model: geometric, Fibonacci-like and random histograms of up to 704 symbols that fit a block never reach debt != 0"""
    rng = np.random.default_rng(1)
    tried = 0
    for n in (17, 24, 64, 256, 704):
        for ratio in (1.05, 1.2, 1.4, 1.6, 1.8, 2.0, 3.0):
            assert limited_depths(_geometric(ratio, n, BLOCK))[0] is not None
            tried += 1
        for _ in range(12):
            cnt = np.maximum(1, (rng.pareto(0.7, n) * 3).astype(np.int64))
            cnt = np.maximum(1, cnt * BLOCK // max(BLOCK, int(cnt.sum())))
            assert limited_depths({s: int(k) for s, k in enumerate(cnt)})[0] is not None
            tried += 1
    for k in range(17, 25):
        assert limited_depths({s: c for s, c in enumerate(_fib(k))})[0] is not None
    assert tried >= 95


GAPS = (1, 2, 3, 10, 11, 13, 14)


def test_zero_runs(T, O):
    """zero runs of 1, 2, 3, 10, 11, 13 and 14 between used literal values, and of hundreds between used command symbols"""
    values, v = [0], 0
    for g in GAPS:
        v += g + 1
        values.append(v)
    c = base(0)
    lit = shuffled({v: 300 + 10 * i for i, v in enumerate(values)}, 4)
    c.lit(lit[:1000]).copy(4, 7000).lit(lit[1000:1500]).copy(300, 7100).lit(lit[1500:1500 + 140]).copy(2118, 7200).lit(lit[1640:1641]).copy(4, 7300)      # command symbols in cells 2, 3, 8 ... hundreds apart
    mb = check(T, O, "zero_runs", c.lit(lit[1641:]).end_block())[1]
    code = mb.lit_codes[0]
    runs = [[(17, 0)] if g == 3 else [(0, 0)] * g if g < 3 else [(17, 7)] + ([(0, 0)] * (g - 10) if g < 14 else [(0, 0), (17, 0)]) for g in GAPS]
    want = [(code.depths[0], 0)]
    for r, v in zip(runs, values[1:]):
        want += r + [(code.depths[v], 0)]
    assert code.cl_symbols == want, code.cl_symbols
    syms = sorted({q.symbol for q in mb.commands})
    assert syms[-1] - syms[0] > 300
    seq = mb.cmd_codes[0].cl_symbols
    assert sum(1 for s, e in seq if (s, e) == (17, 7)) >= 30 and all(not (a[0] == 17 and b[0] == 17) for a, b in zip(seq, seq[1:]))


def test_code_length_code_deeper_than_5(T, O):
    """a description whose code-length symbols have Fibonacci counts: 1 x depth 2, 1 x depth 5, 2 x depth 6, 3 x depth 3, 5 x depth 4 (Kraft sum 1), 8 plain zeros and 13
    zero runs -- five gaps of 14 (17, 0, 17) and three of 11 (17, 0) between the twelve used values.  A Huffman code for these counts is 6 deep (the test's model says so);
    the code-length code holds 5 at most: the branch `maxd > 5`.  No search was needed: seven symbols with Fibonacci counts are the smallest histogram a Huffman code
    takes to depth 6, and the description above has exactly those counts"""
    hist = {2: 1, 5: 1, 6: 2, 3: 3, 4: 5, 0: 8, 17: 13}
    assert max(huffman_depths(hist).values()) == 6
    depth_order = [2, 5, 6, 6, 3, 3, 3, 4, 4, 4, 4, 4]
    gaps = [14, 14, 14, 14, 14, 11, 11, 11, 0, 0, 0]
    counts, v = {}, 0
    for d, g in zip(depth_order, [0] + gaps):
        v += g + (1 if counts else 0)
        counts[v] = 16 << (6 - d)
    mb = check(T, O, "code_length_code_deeper_than_5", _lit_block(base(0), shuffled(counts, 6)))[1]
    code = mb.lit_codes[0]
    assert [code.depths[s] for s in sorted(counts)] == depth_order
    got = {}
    for s_, _ in code.cl_symbols:
        got[s_] = got.get(s_, 0) + 1
    assert got == hist and max(code.clc_lengths) == 5
    print("code-length histogram %r: %d bits, the 5-bit optimum has %d" % (hist, sum(hist[d] * code.clc_lengths[d] for d in hist), package_merge_cost(hist, 5)))


# ---------------------------------------------------------------------------------------------- literal trees
def _context_text(n, seed):
    """bytes whose value depends on what stands in front of them: a digit follows '=', a capital follows ". ", lower case follows letters"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += b"Key" + bytes(rng.integers(97, 123, 3).astype(np.uint8)) + b" = " + bytes(rng.integers(48, 58, 4).astype(np.uint8)) + b". Next " + bytes(rng.integers(97, 101, 5).astype(np.uint8)) + b"\n"
    return bytes(out[:n])


def _tree_check(mb, before=b""):
    """every literal's tree against the RFC's context function (section 7.1, UTF8 mode) and the map the stream states"""
    hist, at = bytearray(before), 0
    for q in mb.commands:
        for t, byte in zip(q.trees, mb.content[at:at + q.insert]):
            p1, p2 = (hist[-1] if len(hist) > 0 else 0), (hist[-2] if len(hist) > 1 else 0)
            assert t == mb.lit_map.map[B.LUT0[p1] | B.LUT1[p2]]
            hist.append(byte)
        hist += mb.content[at + q.insert:at + q.insert + (0 if q.ended else q.copy)]
        at += q.insert + (0 if q.ended else q.copy)


STATIC_MAP = None


def test_thirteen_trees(T, O):
    """context modelling allowed and text whose letters depend on their context: thirteen trees, CONTEXT_UTF8, the static map; the same parse without it: one tree"""
    global STATIC_MAP
    txt = _context_text(20000, 1)
    mb = check(T, O, "thirteen_trees", _lit_block(base(0), txt), ctx=True)[1]
    assert mb.ntreesl == 13 and mb.modes == [B.UTF8] and set(mb.lit_map.map) == set(range(13))
    _tree_check(mb, R[-2:])
    STATIC_MAP = list(mb.lit_map.map)
    # the grouping DESIGN.md names: what follows a line feed, a space, a digit, upper / lower case has a tree of its own
    m = mb.lit_map.map
    ctx = lambda p1, p2: m[B.LUT0[p1] | B.LUT1[p2]]
    assert len({ctx(10, 97), ctx(32, 97), ctx(48, 48), ctx(65, 32), ctx(97, 97)}) == 5
    one = check(T, O, "thirteen_trees_off", _lit_block(base(0), txt), ctx=False)[1]
    assert one.ntreesl == 1 and one.end_bit - one.bit > mb.end_bit - mb.bit


def test_one_tree_is_clear(T, O):
    """context modelling allowed, literals that do not depend on their context: one tree; fewer than 512 literals: one tree whatever they are"""
    mb = check(T, O, "one_tree_flat", _lit_block(base(0), low(20000, 3, 64, 48)), ctx=True)[1]
    assert mb.ntreesl == 1 and mb.modes == [0]
    mb = check(T, O, "one_tree_511", _lit_block(base(0), _context_text(511, 2)), ctx=True)[1]
    assert mb.ntreesl == 1
    mb = check(T, O, "thirteen_trees_2000", _lit_block(base(0), _context_text(2000, 2)), ctx=True)[1]
    assert mb.ntreesl in (1, 13)                                       # (what 2000 literals are worth is the kernel's estimate: not asserted; decodes and codes are checked)


def test_thirteen_trees_first_block_of_a_chunk(T, O):
    """the block under test opens its chunk: stream header, and no bytes in front of the first two literals (context 0, 0)"""
    txt = _context_text(20000, 4)
    c = alone().lit(txt[:8000]).copy(30, 4000).lit(txt[8000:]).end_block()
    mb = check(T, O, "thirteen_trees_first", c, ctx=True)[0]
    assert mb.ntreesl == 13 and mb.bit == 4
    _tree_check(mb)
    assert mb.commands[0].trees[0] == mb.lit_map.map[0]


def test_thirteen_trees_long_runs(T, O):
    """literal runs above 48 in each of the four waves and in the second tile of 256 commands, under thirteen trees (cooperative count, sum and write with contexts)"""
    txt = _context_text(60000, 5)
    c, at = base(0), 0
    for j in range(300):
        ll = 700 if j in (10, 70, 130, 200, 290) else (49 if j in (255, 256) else 20)
        c.lit(txt[at:at + ll]).copy(4, 30000 + j)
        at += ll
    mb = check(T, O, "thirteen_trees_long_runs", c.lit(txt[at:at + 5]).end_block(), ctx=True)[1]
    assert mb.ntreesl == 13 and len(mb.commands) == 301
    _tree_check(mb, R[-2:])


# ---------------------------------------------------------------------------------------------- the bit stream
def test_tile_above_the_window(T, O):
    """a tile of 256 commands above 64 Kbit without a long run (44 random literals and a copy of 20 each): the path through global atomics; one tree and thirteen"""
    rnd = np.random.default_rng(8).integers(0, 256, 48 * 600, dtype=np.uint8).tobytes()
    for ctx in (False, True):
        c, at = base(0), 0
        for j in range(520):
            ll = 40 + j % 9
            c.lit(rnd[at:at + ll] if not ctx else _context_text(ll, j)).copy(20, 50000 + 3 * j)
            at += ll
        mb = check(T, O, "tile_above_the_window_%d" % ctx, c.end_block(), ctx=ctx)[1]
        assert mb.ntreesl == (13 if ctx else 1)
        if not ctx:
            assert mb.commands[256].bit - mb.commands[0].bit > 65536 + 64 and max(q.insert for q in mb.commands) == 48


@pytest.mark.parametrize("run", [48, 49, 256, 257, 5000])
def test_literal_runs(T, O, run):
    """a run of 48 literals is the lane's own, 49 is written by the workgroup; 256 / 257: one and two steps of it; in every wave and in the second tile"""
    c = base(0)
    for j in range(300):
        ll = run if j in (3, 64, 129, 255, 256, 299) and (run < 5000 or j in (3, 256)) else 5
        c.lit(low(ll, j, 32)).copy(3, 40000 + 5 * j)
    mb = check(T, O, "literal_runs_%d" % run, c.lit(low(run, 1)).end_block())[1]
    assert max(q.insert for q in mb.commands) == run


@pytest.mark.parametrize("n,tail", [(1, 0), (255, 1), (256, 0), (257, 3), (513, 0), (MAX_SEQ - 1, 5), (MAX_SEQ, 0)])
def test_command_counts(T, O, n, tail):
    c = base()
    for j in range(n):
        c.lit(b"ab"[j & 1:][:1]).copy(3, 1000 + (j % 7))
    mb = check(T, O, "commands_%d_%d" % (n, tail), c.lit(b"t" * tail).end_block())[1]
    assert len(mb.commands) == n + (1 if tail else 0) and mb.kind == "compressed"


def test_commands_row_full_with_tail(T, O):
    """GC_MAX_SEQ_PER_BLOCK commands and literals behind the last: no entry of the row is left for the tail's command -- the block is stored, the block behind it (whose
    row the tail's entry would have been) is untouched"""
    c = base()
    for j in range(MAX_SEQ):
        c.lit(b"ab"[j & 1:][:1]).copy(3, 1000 + (j % 7))
    c.lit(b"t" * (BLOCK - c.here())).end_block(full=True)
    for j in range(40):
        c.lit(low(3, j)).copy(5, 2000 + j)
    c.stored = {0, 1}
    mbs = check(T, O, "commands_row_full_with_tail", c.end_block())
    assert mbs[1].kind == "stored" and mbs[2].kind == "compressed" and len(mbs[2].commands) == 40


@pytest.mark.parametrize("n", [1, 2, 8, 65536, 65537, 131072])
def test_block_lengths(T, O, n):
    """MNIBBLES 4 up to 65536 and 5 from 65537 (asserted for every block of every case); 1, 2 and 8 bytes are stored"""
    c = base(0)
    c.stored = {0, 1} if n <= 8 else {0}
    if n > 8:
        c.lit(low(n - 1000, 1)).copy(1000, 4321)
    else:
        c.lit(low(n, 1))
    mb = check(T, O, "block_length_%d" % n, c.end_block())[1]
    assert mb.mlen == n and mb.nibbles == (4 if n <= 65536 else 5)


def test_shortest_compressed(T, O):
    """one block alone, a byte and a copy of the rest at distance 1: stored while bits + 64 >= 8 * length; one threshold, and the compressed one obeys the rule"""
    kinds = {}
    for n in range(3, 40):
        c = alone().lit(b"A").copy(n - 1, 1)
        c.stored = None
        x = c.end_block().x()
        s = T.encode(x, P.rows(x, c.blocks))
        st = I.inspect(I.frames(s)[0][2])
        assert st.content == x.tobytes()
        kinds[n] = st.blocks[0].kind
        if kinds[n] == "compressed":
            assert st.blocks[0].end_bit + 64 < 8 * n
    first = min(n for n, k in kinds.items() if k == "compressed")
    assert all(kinds[n] == ("stored" if n < first else "compressed") for n in kinds) and first == 18, kinds
    c = alone().lit(b"A").copy(first - 1, 1)
    check(T, O, "shortest_compressed", c.end_block())
    c = alone().lit(b"A").copy(first - 2, 1)
    c.stored = {0}
    check(T, O, "longest_stored", c.end_block())


def test_stored_in_a_later_tile(T, O):
    """stored chosen in the tile loop: by the first tile (random bytes: block 0 of every case) and by the second (300 cheap commands, then 100 000 random literals)"""
    c = base(0)
    for j in range(300):
        c.lit(low(2, j)).copy(2, 100000 + 13 * j)
    c.lit(R[:100000]).copy(8, 5).end_block()
    c.stored = {0, 1}
    check(T, O, "stored_in_tile_2", c)


def test_stored_between_compressed(T, O):
    """compressed, stored, compressed: every meta-block starts on a byte (asserted for every case), the stored one's padding is zero (the inspector refuses anything else)"""
    c = alone()
    c.lit(low(BLOCK - 100, 1)).copy(100, 777).end_block(full=True)
    c.lit(R).end_block(full=True)
    c.lit(low(500, 2)).copy(100, BLOCK + 10).lit(b"x").end_block()
    c.stored = {1}
    mbs = check(T, O, "stored_between_compressed", c)
    assert [m.kind for m in mbs] == ["compressed", "stored", "compressed"] and mbs[1].content == R


# ---------------------------------------------------------------------------------------------- framing
def test_chunk_boundary(T, O):
    """level 1: eight blocks per chunk.  Nine blocks: two frames, the compressed size and the hint of each (check() holds both against the input), the second stream has a
    header of its own and copies that reach back to ITS first byte"""
    c = alone().lit(low(BLOCK, 1)).end_block(full=True)
    for _ in range(7):
        c.copy(BLOCK, BLOCK).end_block(full=True)
    c.lit(low(300, 2)).copy(200, 300).lit(b"z").end_block()
    mbs = check(T, O, "chunk_boundary", c, level=1)
    s = mbs[0].stream
    fr = I.frames(s)
    assert [h for _, h, _ in fr] == [17, 1] and len(fr[0][2]) + len(fr[1][2]) + 32 == len(s)
    assert mbs[8].bit == 4 and mbs[8].commands[0].distance == 300


def test_plain_stream_in_three_pieces(T, O):
    """one plain stream coded in three calls: only the first has the stream header, only the last the closing meta-block; the join decodes, and a later piece keeps one tree"""
    txt = _context_text(3 * 9000, 6)
    pieces, xs = [], []
    for k, flags in enumerate((PLAIN | NOT_LAST, PLAIN | NOT_FIRST | NOT_LAST, PLAIN | NOT_FIRST)):
        c = alone().lit(txt[9000 * k:9000 * k + 6000]).copy(50, 3000).lit(txt[9000 * k + 6000:9000 * (k + 1)]).end_block()
        s, x, _ = check(T, O, "plain_piece_%d" % k, c, plain=flags, ctx=True)
        pieces.append((s, c))
        xs.append(x.tobytes())
    whole = b"".join(s for s, _ in pieces)
    st = I.inspect(whole)
    assert st.content == b"".join(xs) and st.size == len(whole)
    assert [b.kind for b in st.blocks] == ["compressed", "metadata"] * 3 + ["empty last"]
    assert [b.ntreesl for b in st.blocks if b.kind == "compressed"] == [13, 1, 1]
    assert np.array_equal(T.dec.code(np.frombuffer(whole, np.uint8), capacity=len(st.content) + 64), np.frombuffer(st.content, np.uint8))
    if O.ref("brotli") is not None:
        assert O.ref_brotli_decompress(np.frombuffer(whole, np.uint8), len(st.content)).tobytes() == st.content
    ring, at = P.Ring(), 0
    for k, (s, c) in enumerate(pieces):
        sk = I.inspect(s, header=(k == 0), wbits=24, prefix=st.content[:at], ring=ring.r, open_end=True)
        assert [b.kind for b in sk.blocks] == ["compressed", "metadata"] + (["empty last"] if k == 2 else [])
        assert sk.blocks[0].bit == (4 if k == 0 else 0) and sk.content == xs[k]
        match_blocks("plain_piece_%d" % k, sk, c.x(), c.blocks, [False], 0, ring, last=(k == 2), first=(k == 0))
        at += len(xs[k])


# ---------------------------------------------------------------------------------------------- the reader itself
def test_inspector_reads_the_pinned_streams(O):
    """every accepted stream of tests/golden/brotli_handmade.npz to the content recorded there"""
    import hashlib
    z = np.load(os.path.join(HERE, "golden", "brotli_handmade.npz"))
    D = O.ref_brotli_dictionary() if O.ref("brotli") is not None else None
    read = 0
    for i in range(int(z["n"])):
        flags = z["flags%d" % i]
        if not flags[0] or (flags[1] and D is None):
            continue
        s = z["stream%d" % i].tobytes()
        parts = I.frames(s) if s[:4] == b"\x50\x2a\x4d\x18" else [(0, 0, s)]
        got = b"".join(I.inspect(p, D).content for _, _, p in parts)
        assert len(got) == int(flags[5]) and hashlib.sha256(got).digest() == bytes(z["sha%d" % i]), bytes(z["name%d" % i]).decode()
        read += 1
    assert read >= 60


def test_inspector_reports_what_the_builder_wrote():
    s = B.Stream(18)
    s.uncompressed(b"0123456789")
    cmds = [dict(literals=b"abcab", copy=6, dist=3), dict(literals=b"", copy=4, dcode=0), dict(literals=b"xyz", copy=3, dcode=5), dict(literals=b"q", copy=69, implicit=True),
            dict(literals=b"tail", copy=2, end=True)]
    s.compressed(cmds, npostfix=1, ndirect=6, lit_map=dict(ntrees=3, map=[(i * 7) % 3 for i in range(64)], rlemax=2, imtf=1), modes=(B.SIGNED,))
    s.metadata(b"skip me")
    s.compressed([dict(literals=b"B" * 20, copy=5, dist=20), dict(literals=b"", copy=9, dcode=1)], last=True, blocks=(dict(n=2, first=(0, 3), switches=[(1, 3, 0), (1, 3, 0)]), None, None),
                 modes=(B.LSB6, B.MSB6), lit_map=dict(ntrees=2, map=[0] * 64 + [1] * 64))
    st = I.inspect(s.bytes())
    assert st.wbits == 18 and st.content == bytes(s.out)
    assert [b.kind for b in st.blocks] == ["stored", "compressed", "metadata", "compressed"]
    a, m, b = st.blocks[1], st.blocks[2], st.blocks[3]
    assert (a.npostfix, a.ndirect, a.modes, a.ntreesl, a.lit_map.rlemax, a.lit_map.imtf) == (1, 6, [B.SIGNED], 3, 2, 1) and a.lit_map.map == [(i * 7) % 3 for i in range(64)]
    assert [(q.insert, q.copy, q.dsym) for q in a.commands] == [(5, 6, B.distance_code_for(3, 1, 6)[0]), (0, 4, 0), (3, 3, 5), (1, 69, "implied"), (4, 2, None)]
    assert [q.distance for q in a.commands[:4]] == s.distances[:4] and a.commands[-1].ended and m.skipped == b"skip me"
    assert b.last and b.nbltypes == (2, 1, 1) and b.modes == [B.LSB6, B.MSB6] and b.cats[0].first == 4 and b.cats[0].switches == [(1, 13), (0, 13)]
    assert sorted(set(b.commands[0].trees)) == [0, 1] and [q.distance for q in b.commands] == s.distances[-2:]
    for code in a.lit_codes + a.cmd_codes + a.dist_codes:
        assert code.kind in ("simple", "complex") and code.bits > 0
    # a complex code as told: lengths, HSKIP, the code-length symbols with a repeat
    w = B.BitWriter()
    B.lengths_code(w, 256, {v: 3 for v in range(8)})
    w.put(0, 32)
    code = I.read_code(I.Bits(w.bytes()), 256)
    assert code.kind == "complex" and code.depths == [3] * 8 + [0] * 248 and [v for v, _ in code.cl_symbols][:1] == [3]


@pytest.mark.parametrize("q", [1, 5, 6, 9, 11])
def test_inspector_reads_the_reference_encoder(O, q):
    if O.ref("brotli") is None:
        pytest.skip("oracle/_ref is not built")
    D = O.ref_brotli_dictionary()
    rng = np.random.default_rng(q)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9)).astype(np.uint8)) for _ in range(300)]
    text = b" ".join(words[i] for i in rng.integers(0, 300, 30000))
    html = b"<html><body>The quick brown fox jumps over the lazy dog. Hello, world! 12345 </body></html>\n" * 40
    seen = set()
    for x in (text, html, bytes(rng.integers(0, 256, 50000).astype(np.uint8)) + text[:70000] + html):
        st = I.inspect(O.ref_brotli_compress(np.frombuffer(x, np.uint8), q, 22).tobytes(), D)
        assert st.content == x and st.wbits == 22
        for b in st.blocks:
            if b.kind == "compressed":
                seen |= {"types"} if max(b.nbltypes) > 1 else set()
                seen |= {"ndirect"} if b.ndirect else set()
                seen |= {"rle"} if b.lit_map.rlemax or b.dist_map.rlemax else set()
                seen |= {"imtf"} if b.lit_map.imtf or b.dist_map.imtf else set()
                seen |= {"dictionary"} if any(c.dictionary for c in b.commands) else set()
    if q >= 5:
        assert "types" in seen and "dictionary" in seen
    if q == 11:
        assert {"ndirect", "rle", "imtf"} <= seen
