"""The parse half of the fused verify + parse kernel (gc_mf_vparse_tile_kernel, both geometries): every wave keeps the exit maps of its 16 segments,
hops through them to the entry lane of each segment and walks the 16 segments at the same time, one lane per segment.  The parse must be, byte for
byte, what the serial walk gave: every stream here equals the stream recorded from the emulator build of the commit before the change
(tests/golden/fused_parse_walk/, written by tools/record_fused_parse_walk.py at that commit), decodes under the reference decoders where they are
built, and the GPU's bytes equal the emulator's.

Sizes.  `3 tiles + 37` is 3 x 8 KiB + 37 bytes on the fast geometry (zstd 1-4, brotli 3) and 3 x 16 KiB + 37 on the wide one (FLZMA2 1): the last tile is
shorter than one segment and no multiple of 64.  An input of one block, though, is served by the block-local finder K1 and never reaches the fused kernel
(lz_frame_arg, gc_api.hip), so every input is also taken with one full 128 KiB block in front of those bytes (`block + 3 tiles + 37`): a two-block call
runs the windowed finder, its second block has the three full tiles and the 37-byte one."""
import os

import numpy as np
import pytest

BLK = 128 * 1024
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_parse_walk")
# (encoder class, level, tile bytes): the users of the fused kernel -- zstd lazy depth as zstd_plan sets it, FLZMA2 on the wide geometry, brotli
CODECS = {"zstd1": ("ZstdEncoder", 1, 8192), "zstd3": ("ZstdEncoder", 3, 8192), "zstd4": ("ZstdEncoder", 4, 8192),
          "flzma2_1": ("Flzma2Encoder", 1, 16384), "brotli3": ("BrotliEncoder", 3, 8192)}
KINDS = ("random", "one-byte", "period7", "text-zipf", "planted")
FRONTS = (0, BLK)


def make_input(O, kind, front, tile):
    n = front + 3 * tile + 37
    rng = np.random.default_rng(20261018)
    if kind == "random":                       # every hop a literal: 64 hops per segment
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "one-byte":                     # capped 64-byte matches at distance 1: a segment is left at the lane it was entered
        return np.full(n, 0x41, dtype=np.uint8)
    if kind == "period7":
        return np.tile(np.arange(7, dtype=np.uint8), n // 7 + 1)[:n].copy()
    if kind == "text-zipf":
        return O.corpus("text-zipf", n)
    assert kind == "planted"                   # a 200-byte copy across the boundary in front of the last full tile: cut there, found again behind it with the same offset
    x = rng.integers(0, 256, n, dtype=np.uint8)
    b = front + 2 * tile
    x[b - 100:b + 100] = x[b - 3100:b - 2900]
    return x


def inputs(O, tile, kinds=KINDS):
    return [("%s@%d" % (kind, front), make_input(O, kind, front, tile)) for front in FRONTS for kind in kinds]


def encode_all(pkg, O, name, kinds=KINDS, **kw):
    cls, level, tile = CODECS[name]
    enc = getattr(pkg, cls)(level=level, **kw)
    try:
        prop = enc.coder_props()[0] if cls == "Flzma2Encoder" else None
        return {key: enc.code(x) for key, x in inputs(O, tile, kinds)}, prop
    finally:
        enc.close()


@pytest.fixture(scope="module")
def emu_streams(pkg, O, emu_lib_path):
    """(codec, kind) -> ({input: stream}, LZMA2 property byte) from the emulator build; computed once, shared by the tests below."""
    cache = {}
    def get(name, kind):
        if (name, kind) not in cache:
            cache[name, kind] = encode_all(pkg, O, name, (kind,), lib_path=emu_lib_path)
        return cache[name, kind]
    return get


def _decodes(O, name, c, x, prop):
    cls = CODECS[name][0]
    if cls == "ZstdEncoder":
        assert np.array_equal(O.port_zstd_decompress(c, x.size), x)
        if O.ref("zstd") is not None:
            assert np.array_equal(O.ref_zstd_decompress(c, x.size), x)
    elif cls == "Flzma2Encoder":
        assert np.array_equal(O.port_lzma2_decode(c, x.size, prop), x)
        if O.ref("flzma2") is not None:
            assert np.array_equal(O.ref_lzma2_decode(c, x.size, prop), x)
    elif O.ref("brotli") is not None:
        assert np.array_equal(O.ref_brotlimt_decompress(c, x.size), x)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CODECS))
def test_emu_streams_equal_the_recorded_streams(O, emu_streams, name, kind):
    streams, prop = emu_streams(name, kind)
    with np.load(os.path.join(GOLDEN, name + ".npz")) as gold:
        assert len(gold.files) == len(KINDS) * len(FRONTS)
        for key, x in inputs(O, CODECS[name][2], (kind,)):
            c = streams[key]
            assert c.size == gold[key].size and np.array_equal(c, gold[key]), (name, key, c.size, gold[key].size)
            _decodes(O, name, c, x, prop)


@pytest.mark.gpu
def test_gpu_bytes_equal_emulator_bytes(pkg, O, graft, emu_streams):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    graft.build_hip()
    for name in sorted(CODECS):
        got, _ = encode_all(pkg, O, name, device=0)
        for kind in KINDS:
            want, _ = emu_streams(name, kind)
            for key in want:
                assert np.array_equal(got[key], want[key]), (name, key, got[key].size, want[key].size)
