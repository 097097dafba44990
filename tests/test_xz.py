"""The .xz container (csrc/gc_xz.h) and the segmented CRC kernels under it (csrc/gc_crc_seg.h): SURVEY.md 8 f2, the third bare-file format.

Oracles: Python's `lzma` (liblzma: independent of this code and of the reference) for every stream this encoder writes and as the source of foreign streams; the reference's
host `7z` (oracle/_ref/host7z) where it has been built; a table-driven CRC-64 written in tests/xz_cases.py and zlib's CRC-32 for the raw checksums.  Every case runs twice:
"emu" = the unmodified kernel source under the SIMT emulator, "gpu" (-m gpu) = the product library on the MI355X."""
import ctypes as C
import lzma
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import xz_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST7Z = os.path.join(ROOT, "oracle", "_ref", "host7z", "7z")
MiB = 1 << 20


class _Emu:
    """buffers are host memory, pointers host pointers"""
    name = "emu"

    def __init__(self, lib_path):
        self.kw = dict(lib_path=lib_path); self.lib_path = lib_path

    def put(self, a, shift=0):
        """-> (handle, pointer): a copy of `a` whose first byte lies `shift` bytes behind a 16-byte boundary"""
        buf = np.empty(a.size + 32 + shift, dtype=np.uint8)
        at = (-buf.ctypes.data) % 16 + shift
        buf[at:at + a.size] = a
        return buf[at:at + a.size], buf.ctypes.data + at

    def empty(self, n, fill=0xA5):
        buf = np.full(max(1, n), fill, dtype=np.uint8)
        return buf, buf.ctypes.data

    def get(self, h):
        return h


class _Gpu:
    name = "gpu"

    def __init__(self):
        self.kw = dict(device=0); self.lib_path = None

    def put(self, a, shift=0):
        import torch
        t = torch.empty(a.size + 32 + shift, dtype=torch.uint8, device="cuda:0")
        at = (-t.data_ptr()) % 16 + shift
        if a.size:
            t[at:at + a.size] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        torch.cuda.synchronize()
        return t[at:at + a.size], t.data_ptr() + at

    def empty(self, n, fill=0xA5):
        import torch
        t = torch.full((max(1, n),), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        return t, t.data_ptr()

    def get(self, h):
        return h.cpu().numpy()


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def env(request, graft):
    if request.param == "emu":
        return _Emu(request.getfixturevalue("emu_lib_path"))
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    graft.build_hip()
    return _Gpu()


@pytest.fixture(scope="module")
def dec(pkg, env):
    d = pkg.XzDecoder(**env.kw)
    yield d
    d.close()


def _arr(b):
    return np.ascontiguousarray(np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b, dtype=np.uint8)


def _seven_zip_t(tmp_path, stream, name="t.xz"):
    """`7z t` of the reference's host on the stream, where that host has been built"""
    if not os.path.exists(HOST7Z):
        return
    p = tmp_path / name
    p.write_bytes(bytes(stream))
    r = subprocess.run([HOST7Z, "t", str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "Everything is Ok" in r.stdout, r.stdout[-800:] + r.stderr[-400:]


# ---------------------------------------------------------------------------------------------- 1. CRC-64 raw
def test_crc64_check_vector(pkg, env):
    _, p = env.put(_arr(b"123456789"))
    assert pkg.crc64_device(p, 9, env.lib_path) == 0x995DC9BBDF1939FA
    assert X.crc64(b"123456789") == 0x995DC9BBDF1939FA            # the oracle itself


@pytest.mark.parametrize("n", X.CRC_LENGTHS)
def test_crc64_lengths_fills_and_alignments(pkg, env, n):
    for kind in X.CRC_FILLS:
        want = X.crc64_expected(kind)[n]
        x = X.fill_bytes(kind, X.CRC_LENGTHS[-1])[:n]
        for shift in X.CRC_SHIFTS:
            keep, p = env.put(x, shift)
            got = pkg.crc64_device(p, n, env.lib_path)
            assert got == want, "%s, %d bytes, %d behind a 16-byte boundary: %016x, want %016x" % (kind, n, shift, got, want)


# ---------------------------------------------------------------------------------------------- 2. many segments, one launch
def test_segments_in_one_launch(pkg, env):
    segs, size = X.segment_plan()
    assert 290 <= len(segs) <= 310 and {l for _, l in segs} >= set(X.CRC_LENGTHS) and sum(1 for _, l in segs if l == 0) >= 25 and any(o & 1 for o, _ in segs)
    x = X.fill_bytes("random", size, seed=23)
    x[segs[3][0]:segs[3][0] + 64] = 0                             # a segment that begins with zero bytes
    keep, p = env.put(x)
    enc = pkg.XzEncoder(**env.kw)
    try:
        got64 = enc.segment_checks(p, segs, "crc64")
        got32 = enc.segment_checks(p, segs, "crc32")
    finally:
        enc.close()
    for (o, l), g64, g32 in zip(segs, got64, got32):
        b = x[o:o + l].tobytes()
        assert g32 == (zlib.crc32(b) & 0xFFFFFFFF), (o, l)
        assert g64 == X.crc64(b), (o, l)


# ---------------------------------------------------------------------------------------------- 3. encoder -> liblzma
@pytest.mark.parametrize("block_bytes", X.ENC_BLOCK_BYTES)
@pytest.mark.parametrize("level", X.ENC_LEVELS)
@pytest.mark.parametrize("name", X.ENC_INPUTS)
def test_encoder_streams_decode_with_liblzma(O, pkg, env, dec, tmp_path, name, level, block_bytes):
    x = X.enc_input(O, name)
    prop = pkg.load_library(env.lib_path).gc_flzma2_dict_prop(level)
    for check in X.ENC_CHECKS:
        enc = pkg.XzEncoder(level=level, block_bytes=block_bytes, check=check, **env.kw)
        try:
            c = enc.code(x)
            assert c.size <= enc.compress_bound(x.size)
            assert set(enc.last_timing_ms()) == {"lzma2", "check"}
        finally:
            enc.close()
        assert lzma.decompress(c.tobytes()) == x.tobytes(), (name, level, block_bytes, check)
        if x.size == 0:
            assert c.size == 32
        blocks, nb, units, nu, total = dec.scan(c)
        assert nb == X.expected_blocks(x.size, block_bytes) and total == x.size
        assert all(blocks[i].check == X.CHECK_IDS[check] and blocks[i].dict_prop == prop for i in range(nb))
        _seven_zip_t(tmp_path, c, "%s.xz" % check)


def test_encoder_parameters(O, pkg, env):
    x = _arr(O.corpus("text-zipf", 20_000))
    for bad in (1, 4095):
        enc = pkg.XzEncoder(block_bytes=bad, **env.kw)
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
            enc.code(x)
        enc.close()
    enc = pkg.XzEncoder(check=10, **env.kw)                        # SHA-256: not written
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_PARAM"):
        enc.code(x)
    enc.close()
    enc = pkg.XzEncoder(block_bytes=5001, check="crc32", **env.kw)                  # blocks that start at odd addresses
    c = enc.code(x); enc.close()
    assert lzma.decompress(c.tobytes()) == x.tobytes()


# ---------------------------------------------------------------------------------------------- 4. decoder <- foreign encoders
def _small_mix(O):
    return np.concatenate([O.corpus("text-zipf", 60_000), O.corpus("random", 20_000), np.zeros(30_000, dtype=np.uint8), O.corpus("silesia-like", 40_000)])


@pytest.mark.parametrize("check", X.ENC_CHECKS)
def test_decoder_liblzma_single_block(O, dec, check):
    x = _small_mix(O)
    streams = [lzma.compress(x.tobytes(), format=lzma.FORMAT_XZ, check=X.LZMA_CHECKS[check], preset=p) for p in (0, 6, 9)]
    streams += [lzma.compress(x.tobytes(), format=lzma.FORMAT_XZ, check=X.LZMA_CHECKS[check], filters=[{"id": lzma.FILTER_LZMA2, "preset": 6, "lc": lc, "lp": lp, "pb": pb}])
                for lc, lp, pb in ((4, 0, 0), (0, 2, 2))]
    for s in streams:
        blocks, nb, units, nu, total = dec.scan(_arr(s))
        assert nb == 1 and total == x.size and blocks[0].check == X.CHECK_IDS[check]
        assert dec.code(_arr(s)).tobytes() == x.tobytes()


def _check_layout(dec, stream, layouts):
    """layouts: [(the stream's offset in the file, its layout from X.build_stream)]"""
    blocks, nb, units, nu, total = dec.scan(_arr(stream))
    flat = [(base, l) for base, lay in layouts for l in lay]
    assert nb == len(flat) and total == sum(l["dst_size"] for _, l in flat)
    dst = 0; u = 0
    for i, (base, l) in enumerate(flat):
        b = blocks[i]
        assert (b.src_off, b.src_size, b.dst_off, b.dst_size, b.check_off, b.dict_prop) == (base + l["src_off"], l["src_size"], dst, l["dst_size"], base + l["check_off"], l["dict_prop"])
        assert b.first_unit == u and all(b.src_off <= units[k].src_off and units[k].src_off + units[k].src_size <= b.src_off + b.src_size for k in range(u, u + b.n_units))
        assert sum(units[k].dst_size for k in range(u, u + b.n_units)) == b.dst_size and (b.n_units == 0 or units[u].dst_off == dst)
        dst += l["dst_size"]; u += b.n_units
    assert u == nu
    return nb, nu


@pytest.mark.parametrize("n_blocks", [1, 2, 37])
@pytest.mark.parametrize("check", ["crc64", "crc32"])
def test_decoder_multi_block_files(O, dec, tmp_path, n_blocks, check):
    x = O.corpus("silesia-like", 190_000)
    stream, layout = X.build_stream(X.split_parts(x, n_blocks), check)
    assert lzma.decompress(stream) == x.tobytes()                  # the fixture itself is a legal file
    assert len({l["dict_prop"] for l in layout}) == min(n_blocks, 3)
    nb, nu = _check_layout(dec, stream, [(0, layout)])
    assert dec.code(_arr(stream)).tobytes() == x.tobytes()
    # the parallelism is real: ONE decode launch set over all units, ONE check launch
    assert dec.launch_counts() == (1, nu, 1) and nu >= n_blocks
    _seven_zip_t(tmp_path, stream)


def test_decoder_concatenated_streams_and_padding(O, dec):
    x = O.corpus("text-zipf", 90_000); y = O.corpus("silesia-like", 50_000)
    a, la = X.build_stream(X.split_parts(x, 3), "crc64")
    b, lb = X.build_stream(X.split_parts(y, 2), "crc32")           # another kind of check: a launch of its own
    both = a + b
    assert lzma.decompress(both) == x.tobytes() + y.tobytes()
    _check_layout(dec, both, [(0, la), (len(a), lb)])
    assert dec.code(_arr(both)).tobytes() == x.tobytes() + y.tobytes()
    assert dec.launch_counts()[0] == 1 and dec.launch_counts()[2] == 2
    for pad_mid, pad_end in ((4, 0), (8, 4), (0, 8), (4, 8)):      # liblzma's one-shot decoder takes no padding: against the known input only
        f = a + bytes(pad_mid) + b + bytes(pad_end)
        _check_layout(dec, f, [(0, la), (len(a) + pad_mid, lb)])
        assert dec.code(_arr(f)).tobytes() == x.tobytes() + y.tobytes()
    for f in (a + bytes(3) + b, a + bytes(2), bytes(4) + a):       # padding that is no multiple of four, or in front of the first stream
        with pytest.raises(Exception, match="GC_ERR_CORRUPT"):
            dec.code(_arr(f))
    foreign = lzma.compress(x.tobytes()) + lzma.compress(y.tobytes(), check=lzma.CHECK_NONE)
    assert dec.code(_arr(foreign)).tobytes() == x.tobytes() + y.tobytes()


def test_decoder_zero_block_stream(dec):
    empty, _ = X.build_stream([], "crc64")
    assert len(empty) == 32 and lzma.decompress(empty) == b""
    for s in (empty, lzma.compress(b""), empty + empty):
        blocks, nb, units, nu, total = dec.scan(_arr(s))
        assert (nb, nu, total) == (0, 0, 0) and dec.code(_arr(s)).size == 0
    blk, lay = X.build_stream([(b"", 1 << 16, True)], "crc64")      # (liblzma writes no block for no input; a block of no content made here)
    assert lzma.decompress(blk) == b"" and dec.scan(_arr(blk))[1] == 1 and dec.code(_arr(blk)).size == 0


def test_decoder_seven_zip_multithreaded(O, dec, tmp_path):
    if not os.path.exists(HOST7Z):
        pytest.skip("reference host not built (oracle/_ref/host7z)")
    x = O.corpus("silesia-like", 3 * MiB)
    (tmp_path / "in.bin").write_bytes(x.tobytes())
    r = subprocess.run([HOST7Z, "a", "-txz", "-mmt=4", str(tmp_path / "out.xz"), str(tmp_path / "in.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-400:]
    s = (tmp_path / "out.xz").read_bytes()
    assert dec.scan(_arr(s))[4] == x.size
    assert dec.code(_arr(s)).tobytes() == x.tobytes()


# ---------------------------------------------------------------------------------------------- 5. own round trip through pointers only
def test_round_trip_on_the_device(O, pkg, env, dec):
    x = O.corpus("silesia-like", 2 * X.BLK + 4321)
    src, p_src = env.put(x)
    enc = pkg.XzEncoder(level=5, block_bytes=65536, check="crc64", **env.kw)
    try:
        cap = enc.compress_bound(x.size)
        comp, p_comp = env.empty(cap)
        n = enc.code_device(p_src, x.size, p_comp, cap)
        assert 32 < n <= cap and enc.last_timing_ms()["lzma2"] > 0.0
    finally:
        enc.close()
    stream = env.get(comp)[:n].copy()                              # the host sees the container's headers (the scan) ...
    assert lzma.decompress(stream.tobytes()) == x.tobytes()
    blocks, nb, units, nu, total = dec.scan(stream)
    assert nb == 5 and total == x.size
    out, p_out = env.empty(x.size + 64)
    got = dec.code_device(p_comp, n, p_out, x.size, blocks, nb, units, nu)      # ... and the stored checks are collected on the device
    assert got == x.size and dec.launch_counts() == (1, nu, 1)
    if env.name == "gpu":
        import torch
        assert torch.equal(out[:x.size], src) and bool((out[x.size:] == 0xA5).all())
    else:
        assert np.array_equal(out[:x.size], src) and (out[x.size:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------- 6. refusals
def _refused(pkg, dec, stream, err):
    with pytest.raises(pkg.GpuCodecError, match=err):
        dec.code(_arr(stream))


def _flip(stream, at, bit=0):
    b = bytearray(stream); b[at] ^= 1 << bit
    return bytes(b)


def test_refusals_corrupt(O, pkg, dec):
    x = O.corpus("text-zipf", 50_000)
    s, lay = X.build_stream(X.split_parts(x, 3), "crc64")
    assert dec.code(_arr(s)).tobytes() == x.tobytes()
    n = len(s)
    hdr0 = 12                                                       # the first Block Header
    hdr0_size = (s[hdr0] + 1) * 4
    index_off = lay[-1]["check_off"] + 8
    damaged = {
        "stored CRC-64": _flip(s, lay[1]["check_off"] + 5, 3),
        "stored CRC-64 of the first block": _flip(s, lay[0]["check_off"], 0),
        "block header CRC-32": _flip(s, hdr0 + hdr0_size - 2, 6),
        "block header body": _flip(s, hdr0 + 2, 0),
        "Index CRC-32": _flip(s, n - 12 - 3, 1),
        "Index record": _flip(s, index_off + 3, 2),
        "footer CRC": _flip(s, n - 12, 0), "footer backward size": _flip(s, n - 8, 0), "footer flags": _flip(s, n - 3, 1), "footer magic": _flip(s, n - 1, 0),
        "stream header flags": _flip(s, 7, 0), "stream header magic": _flip(s, 0, 0),
        "truncated in the footer": s[:n - 5], "truncated to a multiple of four": s[:n - 12], "truncated in a block": s[:lay[1]["src_off"] + 10], "nothing": b"",
    }
    for what, bad in damaged.items():
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_CORRUPT"):
            dec.code(_arr(bad)) if len(bad) else dec.scan(_arr(bad))
    # an Index record that disagrees with the payload, in a file whose CRCs are all right: the unpacked size of block 1 one too large, block 2's one too small
    starts = [12] + [l["check_off"] + 8 for l in lay[:-1]]
    recs = [(l["src_off"] - b0 + l["src_size"] + 8, l["dst_size"]) for b0, l in zip(starts, lay)]
    for delta in ((0, 1, -1), (0, 0, 1)):
        index = b"\x00" + X.vli(3) + b"".join(X.vli(u) + X.vli(c + d) for (u, c), d in zip(recs, delta))
        index += bytes(-len(index) % 4); index += struct.pack("<I", zlib.crc32(index))
        assert len(index) == n - 12 - index_off
        _refused(pkg, dec, s[:index_off] + index + s[n - 12:], "GC_ERR_CORRUPT")
    # the content itself: a payload bit flipped where LZMA2 still decodes -- or not: either way the file is refused as damaged
    _refused(pkg, dec, _flip(s, lay[2]["src_off"] + lay[2]["src_size"] // 2, 4), "GC_ERR_CORRUPT")
    assert dec.code(_arr(s)).tobytes() == x.tobytes()              # the context decodes a good file afterwards


def test_refusals_unsupported(O, pkg, dec):
    x = O.corpus("text-zipf", 30_000).tobytes()
    _refused(pkg, dec, lzma.compress(x, check=lzma.CHECK_SHA256), "GC_ERR_UNSUPPORTED")
    delta = lzma.compress(x, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_DELTA, "dist": 4}, {"id": lzma.FILTER_LZMA2, "preset": 6}])
    _refused(pkg, dec, delta, "GC_ERR_UNSUPPORTED")
    bcj = lzma.compress(x, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA2, "preset": 6}])
    _refused(pkg, dec, bcj, "GC_ERR_UNSUPPORTED")
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_UNSUPPORTED"):
        dec.scan(_arr(delta))


def test_refusals_destination_too_small(O, pkg, env, dec):
    x = O.corpus("text-zipf", 40_000)
    s = _arr(lzma.compress(x.tobytes()))
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_DST_SMALL"):
        dec.code(s, capacity=x.size - 1)
    blocks, nb, units, nu, total = dec.scan(s)
    keep, p = env.put(s); out, p_out = env.empty(x.size + 64)
    with pytest.raises(pkg.GpuCodecError, match="GC_ERR_DST_SMALL"):
        dec.code_device(p, s.size, p_out, x.size - 1, blocks, nb, units, nu)
    assert bool((env.get(out) == 0xA5).all())
    enc = pkg.XzEncoder(level=5, block_bytes=8192, **env.kw)
    try:
        full = enc.code(x)
        src, p_src = env.put(x)
        for cap in (0, 11, 12, 40, full.size // 2, full.size - 1):
            dst, p_dst = env.empty(full.size + 64)
            with pytest.raises(pkg.GpuCodecError, match="GC_ERR_DST_SMALL"):
                enc.code_device(p_src, x.size, p_dst, cap)
            assert bool((env.get(dst)[cap:] == 0xA5).all())        # nothing is written behind the capacity
        dst, p_dst = env.empty(full.size)
        assert enc.code_device(p_src, x.size, p_dst, full.size) == full.size and env.get(dst).tobytes() == full.tobytes()
        out = np.empty(full.size, dtype=np.uint8); n = C.c_size_t(0)
        rc = enc._lib.gc_xz_compress_host(enc._ctx, x.ctypes.data, x.size, out.ctypes.data, full.size - 1, 5, 8192, 4, C.byref(n))
        assert rc == -4
    finally:
        enc.close()
