"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against the oracle.

Bit-exactness bars:
  * every compressed stream regenerates the input bit-exactly under the oracle's decoder restatement AND (when
    oracle/_ref travelled with the snapshot) under the reference's own ZSTD_decompress;
  * the GPU's bytes are identical to the bytes the same kernel sources produce under the CPU emulator
    (the encoder is deterministic by construction);
  * compressed size within a stated band of the reference encoder at the same level.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BLK = 128 * 1024
_spec = importlib.util.spec_from_file_location("growth_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "growth_cases.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _roundtrip(O, enc, x):
    c = enc.code(x)
    assert np.array_equal(O.port_zstd_decompress(c, x.size), x)
    if O.ref("zstd") is not None:
        assert np.array_equal(O.ref_zstd_decompress(c, x.size), x)
    return c


def test_native_library_is_the_one_loaded(pkg, gpu_enc):
    maps = open("/proc/self/maps").read()
    assert "7-zip-zstd_amd/csrc/libgpucodec.so" in maps


# levels 1 and 3: the windowed match finder, 8 MiB frames (inputs of one block: the block-local kernel)
@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 8, 63, 64, 255, 256, 1000, 4097, BLK - 1, BLK, BLK + 1, 3 * BLK + 17])
def test_edge_sizes(O, gpu_enc, n, level):
    gpu_enc.set_level(level)
    _roundtrip(O, gpu_enc, O.corpus("text-zipf", n))


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("kind", ["text-zipf", "lz-7zip", "silesia-like", "web-text", "random", "zeros"])
def test_corpora_round_trip_and_ratio(O, gpu_enc, kind, level):
    gpu_enc.set_level(level)
    x = O.corpus(kind, 8 * 1024 * 1024 + 999)
    c = _roundtrip(O, gpu_enc, x)
    if O.ref("zstd") is not None and kind not in ("zeros",):
        ref = O.ref_zstd_compress(x, level)                  # the reference's single stream at the SAME level
        assert len(c) <= 1.02 * len(ref), (kind, level, len(c), len(ref))


@pytest.mark.parametrize("kind", ["text-zipf", "silesia-like", "web-text", "lz-7zip"])
def test_level3_size_within_2_percent_of_reference_stream(O, gpu_enc, kind):
    """The north-star ratio bar: level 3 output within 2 % of the reference's single-stream level-3 size on the same bytes
    (three 8 MiB frames + a partial one)."""
    if O.ref("zstd") is None:
        pytest.skip("oracle/_ref did not travel")
    gpu_enc.set_level(3)
    x = O.corpus(kind, 28 * 1024 * 1024 + 12345)
    c = _roundtrip(O, gpu_enc, x)
    ref = O.ref_zstd_compress(x, 3)
    assert len(c) <= 1.02 * len(ref), (kind, len(c), len(ref))


@pytest.mark.parametrize("level", [1, 3])
def test_gpu_bytes_equal_emulator_bytes(O, gpu_enc, emu_enc, level):
    gpu_enc.set_level(level); emu_enc.set_level(level)
    for kind in ("text-zipf", "silesia-like", "lz-7zip"):
        x = O.corpus(kind, 2 * BLK + 1234)
        assert np.array_equal(gpu_enc.code(x), emu_enc.code(x)), kind
    emu_enc.set_level(3)


@pytest.mark.parametrize("level", [1, 3])
def test_special_patterns(O, gpu_enc, level):
    gpu_enc.set_level(level)
    _roundtrip(O, gpu_enc, O.corpus("zeros", 9 * 1024 * 1024))                  # byte runs across frame boundaries
    z = O.corpus("text-zipf", 3 * 1024 * 1024)
    _roundtrip(O, gpu_enc, np.concatenate([z, z, z, z[:12345]]))                # 3 MiB period: far matches, second frame starts mid-copy
    x = np.tile(np.arange(7, dtype=np.uint8), (4 * BLK) // 7 + 1)[:4 * BLK].copy()
    _roundtrip(O, gpu_enc, x)
    r = O.corpus("random", 70_000)
    _roundtrip(O, gpu_enc, np.concatenate([r, r[:50_000]]))
    rng = np.random.default_rng(7)
    p = 1.0 / np.arange(1, 257) ** 1.2; p /= p.sum()
    _roundtrip(O, gpu_enc, rng.choice(256, size=3 * BLK, p=p).astype(np.uint8))


def test_deterministic_across_calls(O, gpu_enc):
    gpu_enc.set_level(3)
    x = O.corpus("silesia-like", 4 * 1024 * 1024)
    a = gpu_enc.code(x); b = gpu_enc.code(x)
    assert np.array_equal(a, b)


def test_device_pointer_api_full_size(O, gpu_enc):
    """BASELINE config 2 size (100 MB) through the device-pointer entry, checked by the reference decoder."""
    import torch
    gpu_enc.set_level(3)
    n = 100_000_000
    x = O.corpus("text-zipf", n)
    d_src = torch.from_numpy(x).to("cuda:0")
    cap = gpu_enc.compress_bound(n)
    d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_enc.code_device(d_src.data_ptr(), n, d_dst.data_ptr(), cap)
    size = gpu_enc.finish()
    comp = d_dst[:size].cpu().numpy()
    dec = O.ref_zstd_decompress(comp, n) if O.ref("zstd") is not None else O.port_zstd_decompress(comp, n)
    assert np.array_equal(dec, x)
    t = gpu_enc.last_timing_ms()
    assert t["total"] > 0
    assert gpu_enc.mf_timing_ms() is not None          # level 3 ran the windowed finder
    # frames are independent: the stream of a frame-aligned slice is a prefix of the whole stream (sharding property)
    FR = 64 * BLK
    c1 = gpu_enc.code(x[:FR])
    assert np.array_equal(c1, comp[:c1.size])
    assert np.array_equal(O.port_zstd_decompress(c1, FR), x[:FR])


def test_dst_too_small_is_reported(O, gpu_enc, pkg):
    import torch
    x = O.corpus("random", 2 * BLK)
    d_src = torch.from_numpy(x).to("cuda:0")
    d_dst = torch.empty(1000, dtype=torch.uint8, device="cuda:0")
    gpu_enc.code_device(d_src.data_ptr(), x.size, d_dst.data_ptr(), 1000)
    with pytest.raises(pkg.GpuCodecError):
        gpu_enc.finish()


@pytest.mark.parametrize("codec", ["zstd", "flzma2", "brotli"])
def test_growing_the_workspace_never_changes_bytes(pkg, O, gpu_enc, emu_lib_path, codec):
    """small -> large -> small through ONE encoder of the product library: each stream equals a fresh encoder's (tests/growth_cases.py), the large one equals the
    emulator's, and the zstd / brotli streams go back through ONE decoder on the same device in the same order, so that the decoders' workspaces grow as well."""
    streams = G.check_growth_keeps_bytes(pkg, O, codec, device=0)
    cls, level = getattr(pkg, G.CODECS[codec][0]), G.CODECS[codec][1]
    emu = cls(level=level, lib_path=emu_lib_path)
    try:
        large = dict((k.split()[0], x) for k, x in G.inputs(O))["large"]
        assert np.array_equal(streams["large"], emu.code(large)), codec
    finally:
        emu.close()
    if codec != "flzma2":
        dec = (pkg.ZstdDecoder if codec == "zstd" else pkg.BrotliDecoder)(device=0)
        try:
            for name, x in G.inputs(O):
                assert np.array_equal(dec.code(streams[name.split()[0]]), x), (codec, name)
        finally:
            dec.close()
