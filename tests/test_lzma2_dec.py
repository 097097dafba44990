"""The LZMA2 decoder on the device (csrc/gc_lzma2_dec.h; SURVEY.md 8 f1, method id 0x21): one wave per UNIT, a run of chunks from one dictionary reset to the next.

The oracle is always the input itself; on the accepted streams the plain-C restatement (oracle/lzma2_dec.c) and the reference's Lzma2Dec.c must agree.  Three independent
encoders supply streams: the reference's Fast-LZMA2, this engine's own, and xz's (Python's `lzma`, raw LZMA2 -- also stored as tests/golden/lzma2_xz_vectors.npz).
CPU tests run the unmodified kernel source under the SIMT emulator; -m gpu tests run the product library on the MI355X."""
import hashlib
import os
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 128 * 1024
MiB = 1 << 20
END = np.zeros(1, dtype=np.uint8)


def _need_ref(O):
    if O.ref("flzma2") is None:
        pytest.skip("oracle/_ref not built")


@pytest.fixture(scope="module")
def emu_dec(pkg, emu_lib_path):
    d = pkg.Lzma2Decoder(lib_path=emu_lib_path)
    yield d
    d.close()


@pytest.fixture(scope="module")
def gpu_dec(pkg, graft):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    graft.build_hip()
    d = pkg.Lzma2Decoder(device=0)
    yield d
    d.close()


def _arr(c):
    return np.ascontiguousarray(np.frombuffer(c, dtype=np.uint8) if not isinstance(c, np.ndarray) else c, dtype=np.uint8)


def _check(O, dec, comp, prop, want):
    comp = _arr(comp)
    got = dec.code(comp, prop)
    assert got.size == want.size and got.tobytes() == want.tobytes()
    assert O.port_lzma2_decode(comp, want.size, prop).tobytes() == want.tobytes()
    if O.ref("flzma2") is not None:
        assert O.ref_lzma2_decode(comp, want.size, prop).tobytes() == want.tobytes()


def _walk(c):
    """The chunk headers of a stream, written here: [(offset, control, header bytes, unpacked, packed payload)], whether 0x00 was reached."""
    c = bytes(c); off = 0; out = []
    while off < len(c):
        ctl = c[off]
        if ctl == 0:
            return out, True
        if ctl < 0x80:
            u = ((c[off + 1] << 8) | c[off + 2]) + 1
            out.append((off, ctl, 3, u, u)); off += 3 + u
        else:
            hdr = 6 if ctl & 0x40 else 5
            u = (((ctl & 0x1F) << 16) | (c[off + 1] << 8) | c[off + 2]) + 1
            p = ((c[off + 3] << 8) | c[off + 4]) + 1
            out.append((off, ctl, hdr, u, p)); off += hdr + p
    return out, False


def _units_of(chunks):
    units = []
    for off, ctl, hdr, u, p in chunks:
        if ctl == 1 or ctl >= 0xE0:
            units.append(dict(src_off=off, src_size=0, dst_size=0, n_chunks=0))
        units[-1]["src_size"] += hdr + p; units[-1]["dst_size"] += u; units[-1]["n_chunks"] += 1
    return units


def _xz(x, lc=3, lp=0, pb=2, dict_size=1 << 20, preset=6):
    lzma = pytest.importorskip("lzma")
    return _arr(lzma.compress(_arr(x).tobytes(), format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": preset, "lc": lc, "lp": lp, "pb": pb, "dict_size": dict_size}]))


def _dict_prop(size):
    for p in range(40):
        if ((2 | (p & 1)) << (p // 2 + 11)) >= size:
            return p
    return 40


def _mix(O, scale=1):
    """text + bytes that do not compress + zeros + text again: xz writes the chunk kinds 0xE0, 0x80, 0xA0 and 0x02 for it"""
    t = O.corpus("text-zipf", 300_000 * scale)
    return np.concatenate([t, O.corpus("random", 250_000 * scale), np.zeros(400_000 * scale, dtype=np.uint8), t[:300_000 * scale]])


# ---------------------------------------------------------------------------------------------- 1. scan (host code; the emulator library carries it)
def test_scan_units_offsets_and_sizes(O, pkg, emu_dec, emu_lib_path):
    enc = pkg.Flzma2Encoder(lib_path=emu_lib_path, level=5)
    try:
        x = O.corpus("silesia-like", BLK + 5000)
        parts = [enc.code(x[:BLK], flags=enc.NO_END_MARK), enc.code(x[BLK:], flags=enc.NO_END_MARK), enc.code(O.corpus("random", 70_000), flags=enc.NO_END_MARK)]
    finally:
        enc.close()
    c = np.concatenate(parts + [_xz(O.corpus("text-zipf", 40_000), 4, 0, 0)])
    chunks, ended = _walk(c)
    want = _units_of(chunks)
    assert ended and len(want) >= 4
    units, n, total, used, end = emu_dec.scan(c)
    assert n == len(want) and end and used == c.size and total == sum(u["dst_size"] for u in want)
    dst = 0
    for i, w in enumerate(want):
        u = units[i]
        assert (u.src_off, u.src_size, u.dst_off, u.dst_size, u.n_chunks) == (w["src_off"], w["src_size"], dst, w["dst_size"], w["n_chunks"])
        assert bool(u.flags & 0x100) == (i == n - 1)
        dst += w["dst_size"]
    assert units[n - 1].flags & 7 == 4 and all(units[i].flags & 7 <= 4 for i in range(n))
    assert any(ch[1] == 1 for ch in chunks)                       # the random shard starts with a stored chunk that resets the dictionary
    # bytes behind the end marker are not consumed
    _, n2, _, used2, end2 = emu_dec.scan(np.concatenate([c, np.frombuffer(b"\x07trailing", dtype=np.uint8)]))
    assert (n2, used2, end2) == (n, c.size, True)
    # an input cut inside a unit gives the whole units in front of it; a unit is whole once the next dictionary reset has been seen
    for cut in (want[2]["src_off"] + 1, want[2]["src_off"] + want[2]["src_size"] // 2, want[2]["src_off"] + want[2]["src_size"]):
        _, nc, tc, uc, ec = emu_dec.scan(c[:cut])
        assert (nc, uc, ec) == (2, want[2]["src_off"], False) and tc == want[0]["dst_size"] + want[1]["dst_size"]
    _, nc, _, uc, ec = emu_dec.scan(c[:want[2]["src_off"]])
    assert (nc, uc, ec) == (1, want[1]["src_off"], False)         # the second unit's end has not been seen yet
    _, nc, _, uc, ec = emu_dec.scan(c[:c.size - 1])
    assert (nc, uc, ec) == (n - 1, want[n - 1]["src_off"], False)
    assert emu_dec.scan(END)[1:] == (0, 0, 1, True) and emu_dec.scan(np.empty(0, dtype=np.uint8))[1:] == (0, 0, 0, False)


@pytest.mark.parametrize("name,head", [
    ("control 0x03", bytes([0x03, 0, 0])), ("control 0x7F", bytes([0xE0, 0, 0, 0, 5, 0x5D]) + bytes(6) + bytes([0x7F])),
    ("first chunk 0x02", bytes([0x02, 0, 0, 65])), ("first chunk 0x80", bytes([0x80, 0, 0, 0, 5]) + bytes(6)), ("first chunk 0xC0", bytes([0xC0, 0, 0, 0, 5, 0x5D]) + bytes(6)),
    ("no props behind 0x01", bytes([0x01, 0, 0, 65, 0x80, 0, 0, 0, 5]) + bytes(6)), ("no props behind 0x01 0x02", bytes([0x01, 0, 0, 65, 0x02, 0, 0, 66, 0xA0, 0, 0, 0, 5]) + bytes(6)),
    ("props 225", bytes([0xE0, 0, 0, 0, 5, 225]) + bytes(6)), ("lc + lp = 5", bytes([0xE0, 0, 0, 0, 5, 4 + 9 * 1]) + bytes(6)), ("lc 8", bytes([0xE0, 0, 0, 0, 5, 8]) + bytes(6)),
])
def test_scan_refuses_what_lzma2dec_refuses(pkg, emu_dec, name, head):
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_CORRUPT"):
        emu_dec.scan(np.frombuffer(head + b"\x00", dtype=np.uint8))


def test_scan_accepts_the_neighbouring_headers(emu_dec):
    ok = bytes([0x01, 0, 0, 65, 0xC0, 0, 0, 0, 5, 0x5D]) + bytes(6) + bytes([0x02, 0, 0, 66, 0x80, 0, 0, 0, 5]) + bytes(6) + bytes([0xE0, 0, 0, 0, 5, 4 + 9 * 0]) + bytes(6) + b"\x00"
    units, n, total, used, ended = emu_dec.scan(np.frombuffer(ok, dtype=np.uint8))
    assert (n, total, used, ended) == (2, 5, len(ok), True) and units[0].n_chunks == 4 and units[0].flags & 7 == 3 and units[1].flags & 7 == 4


# ---------------------------------------------------------------------------------------------- 2. reference Fast-LZMA2 streams
def _refused_like_the_oracles(O, pkg, dec, c, prop):
    """FL2_compressCCtx writes the two bytes {0x80, 0x00} for NO input: an LZMA chunk header that does not reset the dictionary, cut short.  Lzma2Dec.c and its plain-C
    restatement refuse it, and this decoder must agree with them (empty content from a valid stream: the end marker alone, and this engine's own empty stream)."""
    assert bytes(c) == b"\x80\x00"
    with pytest.raises(ValueError):
        O.port_lzma2_decode(c, 0, prop)
    with pytest.raises(ValueError):
        O.ref_lzma2_decode(c, 0, prop)
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_CORRUPT"):
        dec.code(c, prop)
    assert dec.code(END, prop).size == 0 and O.port_lzma2_decode(END, 0, prop).size == 0 and O.ref_lzma2_decode(END, 0, prop).size == 0


SIZES = [0, 1, 2, 3, 64, 4097, BLK - 1, BLK, BLK + 1]


@pytest.mark.parametrize("kind,n,level", [("text-zipf", n, 5) for n in SIZES] + [("zeros", n, 5) for n in SIZES[4:]] + [(k, n, 5) for k in ("silesia-like", "lz-7zip", "random") for n in (4097, BLK + 1)]
                         + [(k, 400_000, lv) for k in ("text-zipf", "silesia-like") for lv in (1, 5, 9)] + [(k, 400_000, 5) for k in ("lz-7zip", "random", "zeros")])
def test_emu_reference_streams(O, pkg, emu_dec, kind, n, level):
    _need_ref(O)
    x = O.corpus(kind, n) if n else np.empty(0, dtype=np.uint8)
    c, prop = O.ref_fl2_compress(x, level)
    if n == 0:
        _refused_like_the_oracles(O, pkg, emu_dec, c, prop)
        return
    _check(O, emu_dec, c, prop, x)


# ---------------------------------------------------------------------------------------------- 3. this engine's streams
@pytest.mark.parametrize("level", [1, 5, 9])
def test_emu_own_streams(O, pkg, emu_dec, emu_lib_path, level):
    x = O.corpus("silesia-like", 2 * BLK + 4321)
    enc = pkg.Flzma2Encoder(lib_path=emu_lib_path, level=level)
    try:
        _check(O, emu_dec, enc.code(x), enc.coder_props()[0], x)
        _check(O, emu_dec, enc.code(x[:0]), enc.coder_props()[0], x[:0])
    finally:
        enc.close()


def test_emu_shards_are_units(O, pkg, emu_dec, emu_lib_path):
    x = O.corpus("text-zipf", 3 * BLK + 5000)
    enc = pkg.Flzma2Encoder(lib_path=emu_lib_path, level=5)
    try:
        c = np.concatenate([enc.code(x[:BLK], flags=enc.NO_END_MARK), enc.code(x[BLK:BLK + 777], flags=enc.NO_END_MARK), enc.code(x[BLK + 777:])])
        prop = enc.coder_props()[0]
    finally:
        enc.close()
    assert emu_dec.scan(c)[1] == 3
    _check(O, emu_dec, c, prop, x)
    # streams of two encoders in one: decoded with the largest of their dictionary props
    _need_ref(O)
    y = O.corpus("lz-7zip", 90_000)
    r, rprop = O.ref_fl2_compress(y, 9)
    _check(O, emu_dec, np.concatenate([c[:-1], r]), max(prop, rprop), np.concatenate([x, y]))


def test_emu_stored_segments_and_changing_props_inside_a_unit(O, pkg, emu_dec, emu_lib_path, monkeypatch):
    x = np.concatenate([np.tile(O.corpus("text-zipf", 4096), 32), O.corpus("text-zipf", BLK), O.corpus("text-zipf", 40_000)])      # a block that codes in few words, one that needs many, a short one
    monkeypatch.setenv("GC_FRAME_BLOCKS", "1")
    monkeypatch.setenv("GC_SEG_MERGE", "0")                        # every block a model segment of its own: a state reset (0xC0) with props of its own per block
    enc = pkg.Flzma2Encoder(lib_path=emu_lib_path, level=5)
    c0 = enc.code(x); prop = enc.coder_props()[0]; enc.close()
    kinds = [ch[1] & 0xE0 if ch[1] >= 0x80 else ch[1] for ch in _walk(c0)[0]]
    assert kinds.count(0xC0) >= 2 and emu_dec.scan(c0)[1] == 1
    _check(O, emu_dec, c0, prop, x)
    monkeypatch.setenv("GC_SEG_WORD_CAP", "300000")                # the second block's words outgrow their place: stored chunks in the MIDDLE of the unit, LZMA chunks behind them
    enc = pkg.Flzma2Encoder(lib_path=emu_lib_path, level=5)
    c1 = enc.code(x); enc.close()
    kinds = [ch[1] & 0xE0 if ch[1] >= 0x80 else ch[1] for ch in _walk(c1)[0]]
    assert 0x02 in kinds and kinds.index(0x02) > 0 and 0xC0 in kinds[kinds.index(0x02):] and len(c1) > len(c0)
    _check(O, emu_dec, c1, prop, x)


# ---------------------------------------------------------------------------------------------- 4. xz's encoder: live and from the fixture
def _fixture():
    z = np.load(os.path.join(GOLD, "lzma2_xz_vectors.npz"))
    return [(z["stream%d" % i], [int(v) for v in z["props%d" % i]], int(z["size%d" % i]), z["sha%d" % i].tobytes()) for i in range(int(z["n"]))]


def _check_fixture(O, dec, force=None):
    vs = _fixture()
    assert {tuple(p[:3]) for _, p, _, _ in vs} >= {(3, 0, 2), (4, 0, 0), (0, 4, 4), (2, 2, 1)} and min(p[3] for _, p, _, _ in vs) == 0 and max(p[3] for _, p, _, _ in vs) == 24
    for c, (lc, lp, pb, prop), size, sha in vs:
        if force == 1 and lc + lp > 3:
            continue
        units, n, total, _, ended = dec.scan(c)
        assert n == 1 and ended and total == size and units[0].flags & 7 == lc + lp
        y = dec.code(c, prop)
        assert y.size == size and hashlib.sha256(y.tobytes()).digest() == sha
        assert O.port_lzma2_decode(c, size, prop).tobytes() == y.tobytes()


def test_emu_xz_fixture_vectors(O, emu_dec):
    _check_fixture(O, emu_dec)


@pytest.mark.parametrize("lc,lp,pb,dict_size", [(3, 0, 2, 1 << 20), (4, 0, 0, 4 << 10), (0, 4, 4, 64 << 10), (2, 2, 1, 16 << 20), (0, 0, 0, 1 << 16), (1, 2, 3, 1 << 18)])
def test_emu_xz_live(O, emu_dec, lc, lp, pb, dict_size):
    x = np.concatenate([O.corpus("text-zipf", 60_000), O.corpus("random", 70_000), np.zeros(50_000, dtype=np.uint8), O.corpus("silesia-like", 60_000)])
    c = _xz(x, lc, lp, pb, dict_size)
    assert emu_dec.scan(c)[0][0].flags & 7 == lc + lp
    _check(O, emu_dec, c, _dict_prop(dict_size), x)


def test_emu_xz_chunk_kinds(O, emu_dec):
    x = _mix(O)
    c = _xz(x)
    kinds = {ch[1] & 0xE0 if ch[1] >= 0x80 else ch[1] for ch in _walk(c)[0]}
    assert kinds >= {0xE0, 0x80, 0xA0, 0x02}
    _check(O, emu_dec, c, _dict_prop(1 << 20), x)
    r = np.concatenate([O.corpus("random", 80_000), O.corpus("text-zipf", 30_000)])       # begins with bytes that do not compress: 0x01
    c = _xz(r)
    assert _walk(c)[0][0][1] == 0x01
    _check(O, emu_dec, c, _dict_prop(1 << 20), r)


def test_emu_both_kernel_instances(O, pkg, emu_dec, monkeypatch):
    """The host sends a unit to the instance that holds its largest lc + lp.  The hook forces one instance for every unit: lc + lp <= 3 streams decode through the
    lc + lp = 4 instance; an lc + lp = 4 stream sent to the smaller instance is refused by the kernel (it never writes outside its table)."""
    x = O.corpus("text-zipf", 50_000)
    small, large = _xz(x, 3, 0, 2), _xz(x, 2, 2, 0)
    multi = np.concatenate([small[:-1], large[:-1], small[:-1], large])       # both instances in one call
    _check(O, emu_dec, multi, _dict_prop(1 << 20), np.concatenate([x] * 4))
    monkeypatch.setenv("GC_L2D_INSTANCE", "2")
    _check(O, emu_dec, small, _dict_prop(1 << 20), x)
    _check(O, emu_dec, multi, _dict_prop(1 << 20), np.concatenate([x] * 4))
    _check_fixture(O, emu_dec, force=2)
    monkeypatch.setenv("GC_L2D_INSTANCE", "1")
    _check(O, emu_dec, small, _dict_prop(1 << 20), x)
    _check_fixture(O, emu_dec, force=1)
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
        emu_dec.code(large, _dict_prop(1 << 20))
    monkeypatch.delenv("GC_L2D_INSTANCE")
    _check(O, emu_dec, large, _dict_prop(1 << 20), x)


# ---------------------------------------------------------------------------------------------- 5. matches in every shape
def _shapes(O, scale=1):
    rng = np.random.default_rng(11)
    rnd = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8)
    a = rnd(3000)
    far = rnd(5000)
    parts = [far, a, a[:900],                                      # near: inside the ring
             np.zeros(4000, dtype=np.uint8),                       # period 1: copies that overlap themselves at full length
             np.tile(rnd(3), 700), rnd(40_000 * scale),            # period 3; a literal run longer than the ring
             far[100:4900],                                        # far: behind what the ring has handed over, longer than 64 bytes
             np.tile(rnd(70_000), 2), far[:64], a[5:70], far[4000:]]   # period 70 000; short far matches
    return np.concatenate(parts)


def test_emu_every_match_shape(O, emu_dec, monkeypatch):
    x = _shapes(O)
    for inst in ("1", "2"):
        monkeypatch.setenv("GC_L2D_INSTANCE", inst)               # the two instances have rings of different sizes
        for preset, d in ((6, 1 << 20), (1, 1 << 17)):
            _check(O, emu_dec, _xz(x, 3, 0, 2, d, preset), _dict_prop(d), x)
    monkeypatch.delenv("GC_L2D_INSTANCE")
    if O.ref("flzma2") is not None:
        c, prop = O.ref_fl2_compress(x, 9)
        _check(O, emu_dec, c, prop, x)


# ---------------------------------------------------------------------------------------------- 6. damaged streams
KINDS = ("bit", "cut", "eight", "unpacked+1", "unpacked-1", "capacity-1")


def _damaged(c, rng, kind):
    bad = c.copy()
    chunks = [ch for ch in _walk(c)[0] if ch[1] >= 0x80]
    if kind == "bit":
        bad[int(rng.integers(0, bad.size - 1))] ^= 1 << int(rng.integers(0, 8))
    elif kind == "cut":
        bad = bad[:int(rng.integers(1, bad.size - 1))]
    elif kind == "eight":
        i = int(rng.integers(0, bad.size - 9)); bad[i:i + 8] = rng.integers(0, 256, size=8, dtype=np.uint8)
    elif kind in ("unpacked+1", "unpacked-1"):
        off, ctl, _, u, _ = chunks[int(rng.integers(0, len(chunks)))]
        u = u + (1 if kind == "unpacked+1" else -1)
        if u < 1 or u > (1 << 21):
            return None
        bad[off] = (ctl & 0xE0) | ((u - 1) >> 16); bad[off + 1] = ((u - 1) >> 8) & 0xFF; bad[off + 2] = (u - 1) & 0xFF
    return bad


def _oracles(O, bad, cap, prop):
    """What the independent decoders make of a stream: the content, or None when they refuse it.  The plain-C restatement and (where built) the reference's Lzma2Dec.c
    must say the same."""
    def run(f):
        try:
            return f(bad, cap, prop).tobytes()
        except ValueError:
            return None
    p = run(O.port_lzma2_decode)
    if O.ref("flzma2") is not None:
        r = run(O.ref_lzma2_decode)
        assert (p is None) == (r is None) and p == r, "the two oracles disagree"
    return p


PAYLOAD_KINDS = ("bit", "eight", "unpacked+1", "unpacked-1")


def _damage_round(O, pkg, lib_path, dev, c, prop, x, rng, rounds):
    """Every damaged input goes through this decoder AND the oracles.  Accepted here: the oracles accept it too, with the same bytes (which are the content itself unless
    the damage made another valid stream: LZMA2 carries no checksum).  Refused here as damaged: the oracles refuse it too.  The output buffer behind the produced bytes keeps
    its pattern; the context decodes a good stream afterwards.  -> refusals per kind, and those of them that came from the KERNEL (the header scan had accepted the stream)."""
    dec = pkg.Lzma2Decoder(device=dev, lib_path=lib_path) if lib_path else pkg.Lzma2Decoder(device=dev)
    refused = {k: 0 for k in KINDS}; by_kernel = {k: 0 for k in KINDS}
    import ctypes as C
    try:
        for r in range(rounds):
            kind = KINDS[r % len(KINDS)]
            bad = _damaged(c, rng, kind) if kind != "capacity-1" else c
            if bad is None:
                continue
            cap = x.size - 1 if kind == "capacity-1" else x.size + 4096
            out = np.full(x.size + 8192, 0xA5, dtype=np.uint8)
            n = C.c_size_t(0)
            rc = dec._lib.gc_lzma2_decompress_host(dec._ctx, bad.ctypes.data, bad.size, out.ctypes.data, cap, prop, C.byref(n))
            want = _oracles(O, bad, cap, prop)
            if rc != 0:
                refused[kind] += 1
                assert rc in (-4, -6), rc                          # DST_SMALL or CORRUPT: never a HIP failure, never a parameter error
                assert kind != "capacity-1" or rc == -4
                assert (out == 0xA5).all()                         # (the host entry copies nothing back when the call fails)
                assert want is None, "refused a stream that the oracles decode (%s, rc %d)" % (kind, rc)
                try:
                    scanned = dec.scan(bad)
                    by_kernel[kind] += 1 if scanned[4] and scanned[2] <= cap else 0
                except pkg.GpuCodecError:
                    pass
            else:
                assert kind not in ("cut", "capacity-1")
                assert (out[n.value:] == 0xA5).all()
                assert want is not None and out[:n.value].tobytes() == want, "accepted a stream that the oracles refuse or decode differently (%s)" % kind
                assert kind in ("bit", "eight") or want == x.tobytes()      # (a changed size field cannot give other content of a valid stream)
        assert dec.code(c, prop).tobytes() == x.tobytes()
    finally:
        dec.close()
    return refused, by_kernel


def _device_ranges_keep_their_pattern(dec, c, prop, x, rng, rounds, alloc, fetch):
    """The same through the device entry: units of a damaged stream never write outside [dst_off, dst_off + dst_size) of the buffer they were given."""
    refused = 0
    for r in range(rounds):
        bad = _damaged(c, rng, ("bit", "eight", "unpacked+1", "unpacked-1")[r % 4])
        if bad is None:
            continue
        try:
            units, n, total, used, ended = dec.scan(bad)
        except Exception:
            refused += 1
            continue
        if n == 0:
            continue
        gap = 512
        for i in range(n):                                        # spread the units: a guard band between neighbours
            units[i].dst_off = units[i].dst_off + gap * (i + 1)
        size = int(total) + gap * (n + 2)
        src, dst, d_src, d_dst = alloc(bad, size)
        try:
            dec.code_device(d_src, used, d_dst, size, prop, units, n)
        except Exception:
            refused += 1
        out = fetch(dst)
        covered = np.zeros(size, dtype=bool)
        for i in range(n):
            covered[units[i].dst_off:units[i].dst_off + units[i].dst_size] = True
        assert (out[~covered] == 0xA5).all()
    return refused


def _host_alloc(bad, size):
    dst = np.full(size, 0xA5, dtype=np.uint8)
    return bad, dst, bad.ctypes.data, dst.ctypes.data


def test_emu_damaged_streams_are_refused_or_harmless(O, pkg, emu_lib_path, emu_dec):
    _need_ref(O)
    rng = np.random.default_rng(7)
    x = np.concatenate([O.corpus("text-zipf", 20_000), O.corpus("random", 3_000), O.corpus("silesia-like", 12_000)])
    enc = pkg.Flzma2Encoder(lib_path=emu_lib_path, level=5)
    own = np.concatenate([enc.code(x[:18_000], flags=enc.NO_END_MARK), enc.code(x[18_000:])]); oprop = enc.coder_props()[0]; enc.close()
    ref, rprop = O.ref_fl2_compress(x, 5)
    total = {k: 0 for k in KINDS}; kernel = {k: 0 for k in KINDS}
    for c, prop in ((own, oprop), (ref, rprop), (_xz(x, 2, 2, 1, 1 << 16), _dict_prop(1 << 16))):
        refused, by_kernel = _damage_round(O, pkg, emu_lib_path, 0, c, prop, x, rng, 36)
        for k in KINDS:
            total[k] += refused[k]; kernel[k] += by_kernel[k]
        _device_ranges_keep_their_pattern(emu_dec, c, prop, x, rng, 8, _host_alloc, lambda d: d)
    assert all(v > 0 for v in total.values()), total
    assert all(kernel[k] > 0 for k in PAYLOAD_KINDS), kernel       # each kind of payload damage was caught by the kernel itself, not only by the header scan


# ---------------------------------------------------------------------------------------------- 6b. hand-made LZMA chunks: one for every check the kernel makes by name
class _Enc:
    """A small LZMA encoder written for these tests from the format's description (lc 3, lp 0, pb 2): range coder with carry, literals (plain and matched), matches,
    short reps and rep0 matches.  It codes what it is TOLD to, valid or not; `buf` is what a decoder would have produced so far."""
    def __init__(self):
        self.low = 0; self.range = 0xFFFFFFFF; self.cache = 0; self.pending = 1; self.out = bytearray()
        self.p = {}; self.state = 0; self.rep0 = 0; self.buf = bytearray()

    def _shift(self):
        if self.low < 0xFF000000 or self.low >= (1 << 32):
            carry = self.low >> 32; t = self.cache
            while self.pending:
                self.out.append((t + carry) & 0xFF); t = 0xFF; self.pending -= 1
            self.cache = (self.low >> 24) & 0xFF
        self.pending += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, key, b):
        pr = self.p.get(key, 1024)
        bound = (self.range >> 11) * pr
        if b:
            self.low += bound; self.range -= bound; self.p[key] = pr - (pr >> 5)
        else:
            self.range = bound; self.p[key] = pr + ((2048 - pr) >> 5)
        while self.range < (1 << 24):
            self.range = (self.range << 8) & 0xFFFFFFFF; self._shift()

    def direct(self, v, n):
        for i in range(n - 1, -1, -1):
            self.range >>= 1
            if (v >> i) & 1:
                self.low += self.range
            while self.range < (1 << 24):
                self.range = (self.range << 8) & 0xFFFFFFFF; self._shift()

    def tree(self, name, v, n):
        m = 1
        for i in range(n - 1, -1, -1):
            b = (v >> i) & 1; self.bit((name, m), b); m = (m << 1) | b

    def tree_rev(self, name, v, n):
        m = 1
        for i in range(n):
            b = (v >> i) & 1; self.bit((name, m), b); m = (m << 1) | b

    def _ps(self):
        return len(self.buf) & 3

    def literal(self, byte):
        self.bit(("match", self.state, self._ps()), 0)
        ctx = (self.buf[-1] if self.buf else 0) >> 5
        sym = 1
        if self.state < 7:
            for i in range(7, -1, -1):
                b = (byte >> i) & 1; self.bit(("lit", ctx, sym), b); sym = (sym << 1) | b
        else:
            mb = self.buf[len(self.buf) - self.rep0 - 1] if self.rep0 < len(self.buf) else 0
            offs = 0x100
            for i in range(7, -1, -1):
                mb <<= 1; m = mb & offs; b = (byte >> i) & 1
                self.bit(("lit", ctx, offs + m + sym), b); sym = (sym << 1) | b
                offs &= mb if b else ~mb
        self.buf.append(byte)
        self.state = 0 if self.state < 4 else (self.state - 3 if self.state < 10 else self.state - 6)

    def _len(self, name, n):
        v = n - 2
        if v < 8:
            self.bit((name, "c1"), 0); self.tree((name, "low", self._ps()), v, 3)
        elif v < 16:
            self.bit((name, "c1"), 1); self.bit((name, "c2"), 0); self.tree((name, "mid", self._ps()), v - 8, 3)
        else:
            self.bit((name, "c1"), 1); self.bit((name, "c2"), 1); self.tree((name, "high"), v - 16, 8)

    def _copy(self, n):
        for _ in range(n):
            self.buf.append(self.buf[len(self.buf) - self.rep0 - 1] if self.rep0 < len(self.buf) else 0)

    def match(self, n, dist):                                      # dist = distance - 1
        self.bit(("match", self.state, self._ps()), 1); self.bit(("rep", self.state), 0)
        self._len("len", n)
        slot = dist if dist < 4 else 2 * (dist.bit_length() - 1) + ((dist >> (dist.bit_length() - 2)) & 1)
        self.tree(("slot", min(n - 2, 3)), slot, 6)
        if slot >= 4:
            nd = (slot >> 1) - 1; base = (2 | (slot & 1)) << nd; rem = dist - base
            if slot < 14:
                self.tree_rev(("spec", base - slot), rem, nd)
            else:
                self.direct(rem >> 4, nd - 4); self.tree_rev("align", rem & 15, 4)
        self.rep0 = dist; self.state = 7 if self.state < 7 else 10
        self._copy(n)

    def short_rep(self):
        self.bit(("match", self.state, self._ps()), 1); self.bit(("rep", self.state), 1); self.bit(("g0", self.state), 0); self.bit(("rep0long", self.state, self._ps()), 0)
        self.state = 9 if self.state < 7 else 11
        self._copy(1)

    def rep0_match(self, n):
        self.bit(("match", self.state, self._ps()), 1); self.bit(("rep", self.state), 1); self.bit(("g0", self.state), 0); self.bit(("rep0long", self.state, self._ps()), 1)
        self._len("replen", n)
        self.state = 8 if self.state < 7 else 11
        self._copy(n)

    def payload(self):
        for _ in range(5):
            self._shift()
        return bytes(self.out)


def _chunk(payload, usize, csize=None):
    csize = len(payload) if csize is None else csize
    return bytes([0xE0 | ((usize - 1) >> 16), ((usize - 1) >> 8) & 0xFF, (usize - 1) & 0xFF, ((csize - 1) >> 8) & 0xFF, (csize - 1) & 0xFF, 0x5D]) + payload


def _good(e):
    for b in b"abcabc":
        e.literal(b)
    e.match(40, 2); e.literal(ord("x")); e.short_rep(); e.rep0_match(20); e.match(3, 30); e.literal(ord("y"))


def _hand_made():
    """name -> (stream, what a decoder gives: the content, or None for a refusal)"""
    out = {}
    e = _Enc(); _good(e); good = e.payload(); content = bytes(e.buf)
    out["the encoder's own valid chunk"] = (_chunk(good, len(content)) + b"\x00", content)
    out["first range-coder byte not 0"] = (_chunk(b"\x01" + good[1:], len(content)) + b"\x00", None)
    out["packed size below the coder's five bytes"] = (_chunk(good[:3], 1) + b"\x00", None)
    out["payload left over"] = (_chunk(good + b"\x00", len(content)) + b"\x00", None)
    e = _Enc(); _good(e); e.literal(ord("z")); longer = e.payload()
    out["coder not at rest when the bytes are out"] = (_chunk(longer, len(content)) + b"\x00", None)
    out["input exhausted inside a symbol"] = (_chunk(good, len(content) + 1) + b"\x00", None)
    e = _Enc(); e.literal(ord("a")); e.match(2, 0xFFFFFFFF)
    out["end-of-payload marker"] = (_chunk(e.payload(), 3) + b"\x00", None)
    e = _Enc(); e.literal(ord("a")); e.match(10, 0)
    out["match longer than the chunk's remainder"] = (_chunk(e.payload(), 5) + b"\x00", None)
    e = _Enc(); e.short_rep(); e.literal(ord("a"))
    out["short rep at position 0"] = (_chunk(e.payload(), 2) + b"\x00", None)
    e = _Enc(); e.rep0_match(4); e.literal(ord("a"))
    out["rep match at position 0"] = (_chunk(e.payload(), 5) + b"\x00", None)
    e = _Enc(); e.literal(ord("a")); e.literal(ord("b")); e.match(4, 2); e.literal(ord("c"))
    out["distance beyond the bytes since the dictionary reset"] = (_chunk(e.payload(), 7) + b"\x00", None)
    return out


def _check_hand_made(O, pkg, dec):
    cases = _hand_made()
    assert len(cases) == 11
    for name, (stream, want) in cases.items():
        c = _arr(stream)
        assert dec.scan(c)[4], name                               # the headers are in order: what is wrong is for the kernel to find
        got = _oracles(O, c, 4096, 40)
        assert got == want, "the oracles on: " + name
        if want is None:
            with pytest.raises(pkg.GpuCodecError, match="GC_ERR_CORRUPT"):
                dec.code(c, 40)
        else:
            assert dec.code(c, 40).tobytes() == want, name


def test_emu_hand_made_chunks_hit_every_named_check(O, pkg, emu_dec):
    _check_hand_made(O, pkg, emu_dec)


def test_emu_parameter_checks(O, pkg, emu_dec):
    c = _xz(O.corpus("text-zipf", 3000))
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
        emu_dec.code(c, 41)
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_CORRUPT"):
        emu_dec.code(c[:-1], 40)                                  # no end marker
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_CORRUPT"):
        emu_dec.code(_xz(O.corpus("text-zipf", 30_000), dict_size=1 << 16), 0)      # distances beyond the 4 KiB the property byte states
    units = (pkg.Lzma2Unit * 1)()
    dst = np.zeros(16, dtype=np.uint8)
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
        emu_dec.code_device(c.ctypes.data, c.size, dst.ctypes.data, 16, 40, units, (1 << 20) + 1)
    # units from a caller, not from the scan: an output range behind the capacity, or one whose end wraps around 2^64, is refused before anything runs
    units, n, total, used, _ = emu_dec.scan(c)
    dst = np.full(total + 64, 0xA5, dtype=np.uint8)
    for off in (1, total + 64, (1 << 64) - 8, (1 << 64) - total):
        units[0].dst_off = off
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_DST_SMALL"):
            emu_dec.code_device(c.ctypes.data, used, dst.ctypes.data, total, 40, units, n)
        assert (dst == 0xA5).all()
    units[0].dst_off = 0
    assert emu_dec.code_device(c.ctypes.data, used, dst.ctypes.data, total, 40, units, n) == total
    assert emu_dec.last_timing_ms() >= 0.0


# ---------------------------------------------------------------------------------------------- GPU
def _gpu_check(O, dec, comp, prop, want, port=True):
    comp = _arr(comp)
    got = dec.code(comp, prop)
    assert got.size == want.size and got.tobytes() == want.tobytes()
    if O.ref("flzma2") is not None:
        assert O.ref_lzma2_decode(comp, want.size, prop).tobytes() == want.tobytes()
    elif port:
        assert O.port_lzma2_decode(comp, want.size, prop).tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["text-zipf", "silesia-like", "lz-7zip", "random", "zeros", "real-src", "real-bin"])
@pytest.mark.parametrize("level", [1, 5, 9])
def test_gpu_reference_streams(O, gpu_dec, kind, level):
    _need_ref(O)
    x = O.corpus(kind, 24 * MiB + 12345)
    if x.size < MiB:
        pytest.skip("the image holds no %s data" % kind)
    c, prop = O.ref_fl2_compress(x, level, min(os.cpu_count() or 1, 16))
    _gpu_check(O, gpu_dec, c, prop, x)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_edge_sizes(O, pkg, gpu_dec, n):
    _need_ref(O)
    x = O.corpus("text-zipf", n) if n else np.empty(0, dtype=np.uint8)
    c, prop = O.ref_fl2_compress(x, 5)
    if n == 0:
        _refused_like_the_oracles(O, pkg, gpu_dec, c, prop)
        return
    _gpu_check(O, gpu_dec, c, prop, x)


@pytest.mark.gpu
@pytest.mark.parametrize("level,n,shard", [(5, 64 * MiB, 16 * MiB), (5, 64 * MiB, 0), (1, 24 * MiB + 1, 0), (9, 24 * MiB + 1, 0), (5, 0, 0), (5, 1, 0)])
def test_gpu_own_streams(O, pkg, gpu_dec, level, n, shard):
    x = O.corpus("silesia-like", n) if n else np.empty(0, dtype=np.uint8)
    enc = pkg.Flzma2Encoder(device=0, level=level)
    try:
        if shard:
            c = np.concatenate([enc.code(x[i:i + shard], flags=enc.NO_END_MARK) for i in range(0, n, shard)] + [END])
            assert gpu_dec.scan(c)[1] == n // shard
        else:
            c = enc.code(x)
        prop = enc.coder_props()[0]
    finally:
        enc.close()
    _gpu_check(O, gpu_dec, c, prop, x)


@pytest.mark.gpu
def test_gpu_stored_segments_and_changing_props(O, pkg, gpu_dec, gpu_hooks_kw, monkeypatch):
    # blocks that code in few words (LZMA), blocks of text that need more words than the lowered cap allows (stored), few-word blocks again, incompressible bytes, a short block
    few = np.tile(O.corpus("text-zipf", 4096), 64)
    x = np.concatenate([few, O.corpus("text-zipf", 2 * BLK), few[:BLK], O.corpus("random", BLK), O.corpus("text-zipf", 40_000)])
    monkeypatch.setenv("GC_FRAME_BLOCKS", "1")
    monkeypatch.setenv("GC_SEG_MERGE", "0")
    monkeypatch.setenv("GC_SEG_WORD_CAP", "300000")
    enc = pkg.Flzma2Encoder(level=5, **gpu_hooks_kw)
    c = enc.code(x); prop = enc.coder_props()[0]; enc.close()
    kinds = [ch[1] & 0xE0 if ch[1] >= 0x80 else ch[1] for ch in _walk(c)[0]]
    assert kinds[0] == 0xE0 and 0x02 in kinds and 0xC0 in kinds[kinds.index(0x02):] and kinds.count(0xC0) >= 2
    _gpu_check(O, gpu_dec, c, prop, x)


@pytest.mark.gpu
def test_gpu_xz_vectors_and_instances(O, pkg, gpu_dec, gpu_hooks_kw, monkeypatch):
    _check_fixture(O, gpu_dec)
    x = _mix(O, 4)
    for lc, lp, pb, d in ((3, 0, 2, 1 << 20), (4, 0, 0, 4 << 10), (0, 4, 4, 64 << 10), (2, 2, 1, 16 << 20)):
        _gpu_check(O, gpu_dec, _xz(x, lc, lp, pb, d), _dict_prop(d), x)
    small, large = _xz(x[:MiB], 3, 0, 2), _xz(x[:MiB], 2, 2, 0)
    _gpu_check(O, gpu_dec, np.concatenate([small[:-1], large[:-1], small[:-1], large]), _dict_prop(1 << 20), np.concatenate([x[:MiB]] * 4))
    hooked = pkg.Lzma2Decoder(**gpu_hooks_kw)
    try:
        monkeypatch.setenv("GC_L2D_INSTANCE", "2")
        _gpu_check(O, hooked, small, _dict_prop(1 << 20), x[:MiB])
        _check_fixture(O, hooked, force=2)
        monkeypatch.setenv("GC_L2D_INSTANCE", "1")
        _check_fixture(O, hooked, force=1)
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
            hooked.code(large, _dict_prop(1 << 20))
        y = _shapes(O, 8)
        for inst in ("1", "2"):
            monkeypatch.setenv("GC_L2D_INSTANCE", inst)
            _gpu_check(O, hooked, _xz(y, 3, 0, 2, 1 << 20, 6), _dict_prop(1 << 20), y)
    finally:
        hooked.close()


@pytest.mark.gpu
def test_gpu_damaged_streams_are_refused_or_harmless(O, pkg, gpu_dec):
    _need_ref(O)
    import torch
    rng = np.random.default_rng(8)
    x = np.concatenate([O.corpus("text-zipf", 300_000), O.corpus("random", 70_000), O.corpus("silesia-like", 200_000)])
    enc = pkg.Flzma2Encoder(device=0, level=5)
    own = np.concatenate([enc.code(x[:250_000], flags=enc.NO_END_MARK), enc.code(x[250_000:])]); oprop = enc.coder_props()[0]; enc.close()
    ref, rprop = O.ref_fl2_compress(x, 5)
    keep = []

    def alloc(bad, size):
        s = torch.from_numpy(bad).to("cuda:0"); d = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize(); keep[:] = [s, d]
        return s, d, s.data_ptr(), d.data_ptr()
    total = {k: 0 for k in KINDS}; kernel = {k: 0 for k in KINDS}
    for c, prop in ((own, oprop), (ref, rprop), (_xz(x, 2, 2, 1, 1 << 16), _dict_prop(1 << 16))):
        refused, by_kernel = _damage_round(O, pkg, None, 0, c, prop, x, rng, 60)
        for k in KINDS:
            total[k] += refused[k]; kernel[k] += by_kernel[k]
        _device_ranges_keep_their_pattern(gpu_dec, c, prop, x, rng, 12, alloc, lambda d: d.cpu().numpy())
    assert all(v > 0 for v in total.values()), total
    assert all(kernel[k] > 0 for k in PAYLOAD_KINDS), kernel


@pytest.mark.gpu
def test_gpu_hand_made_chunks_hit_every_named_check(O, pkg, gpu_dec):
    _check_hand_made(O, pkg, gpu_dec)


@pytest.mark.gpu
def test_gpu_device_api_encoder_to_decoder_in_hbm(O, pkg, gpu_dec):
    """FLZMA2 encoder -> LZMA2 decoder on the device: the host sees the compressed bytes' chunk headers (the scan) and never the content."""
    import torch
    n = 48 * MiB
    x = O.corpus("silesia-like", n)
    d_src = torch.from_numpy(x).to("cuda:0")
    enc = pkg.Flzma2Encoder(device=0, level=5)
    try:
        shard = 16 * MiB
        cap = enc.compress_bound(shard)
        d_comp = torch.empty(3 * cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        at = 0
        for i in range(3):
            enc.code_device(d_src.data_ptr() + i * shard, shard, d_comp.data_ptr() + at, cap, flags=enc.NO_END_MARK)
            at += enc.finish()
        d_comp[at] = 0; at += 1
        prop = enc.coder_props()[0]
    finally:
        enc.close()
    units, nu, total, used, ended = gpu_dec.scan(d_comp[:at].cpu().numpy())
    assert (nu, total, used, ended) == (3, n, at, True)
    d_out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    got = gpu_dec.code_device(d_comp.data_ptr(), used, d_out.data_ptr(), n, prop, units, nu)
    assert got == n and torch.equal(d_out[:n], d_src) and bool((d_out[n:] == 0xA5).all())
    assert gpu_dec.last_timing_ms() > 0.0


@pytest.mark.gpu
def test_gpu_units_run_side_by_side(O, gpu_dec):
    """64 units of 1 MiB against the same unit alone, minimum of three timings each.  64 waves on 256 CUs should take about 1 x t1, a decoder that serialises its units
    takes 64 x t1; 8 leaves room for clocks and a busy machine while still telling the two apart."""
    _need_ref(O)
    import torch
    x = O.corpus("text-zipf", MiB)
    c, prop = O.ref_fl2_compress(x, 5)
    assert gpu_dec.scan(c)[1] == 1

    def timed(comp, copies):
        d_src = torch.from_numpy(comp).to("cuda:0")
        units, nu, total, used, _ = gpu_dec.scan(comp)
        assert nu == copies and total == copies * MiB
        d_out = torch.empty(total + 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ts = []
        for _ in range(4):                                        # (the first call warms up)
            assert gpu_dec.code_device(d_src.data_ptr(), used, d_out.data_ptr(), total, prop, units, nu) == total
            ts.append(gpu_dec.last_timing_ms())
        want = torch.from_numpy(x).to("cuda:0")
        for k in (0, copies // 2, copies - 1):
            assert torch.equal(d_out[k * MiB:(k + 1) * MiB], want)
        return min(ts[1:])
    t1 = timed(c, 1)
    t64 = timed(np.concatenate([c[:-1]] * 64 + [END]), 64)
    print("t1 = %.3f ms, t64 = %.3f ms, t64 / t1 = %.2f" % (t1, t64, t64 / t1))
    assert t64 < 8 * t1
