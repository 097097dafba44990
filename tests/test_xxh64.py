"""gc_xxh64_device (the device code of the zstd content checksums over one "frame" of n bytes) against the oracle's gco_xxh64, on the emulator and on the device.
The lengths and why they are the ones: tests/zstd_checksum_cases.py."""
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("zstd_checksum_cases", os.path.join(HERE, "zstd_checksum_cases.py"))
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)

LENGTH_CASES = [(n, 0) for n in K.XXH_LENGTHS] + [(K.XXH_OFFSET_LEN, off) for off in K.XXH_OFFSETS]


def _want(O, a, seed):
    a = np.ascontiguousarray(a)
    return O.port().gco_xxh64(a.ctypes.data if a.size else None, a.size, seed)


def test_tile_of_the_cases_is_the_kernels():
    text = open(os.path.join(ROOT, "7-zip-zstd_amd", "csrc", "gc_common.h")).read()
    assert int(re.search(r"#define\s+GC_XXH64_TILE\s+(\d+)u", text).group(1)) == K.T


def test_abi_has_the_checksum_surface_emulator(pkg, emu_lib_path):
    lib = pkg.load_library(emu_lib_path)
    assert hasattr(lib, "gc_xxh64_device") and hasattr(lib, "gc_zstd_checksum_timing")
    e = pkg.ZstdEncoder(lib_path=emu_lib_path)
    assert lib.gc_ctx_set_option(e._ctx, 3, 1) == pkg.GC_OK
    assert lib.gc_ctx_set_option(e._ctx, 3, 0) == pkg.GC_OK
    assert lib.gc_ctx_set_option(e._ctx, 4, 1) == -5                         # GC_ERR_PARAM: still no such option
    e.close()


@pytest.mark.parametrize("data,want", K.XXH_KNOWN)
def test_known_answers_emulator(pkg, emu_lib_path, data, want):
    a = np.frombuffer(data + b"\0", dtype=np.uint8)                          # (one spare byte: a pointer to hand over for the empty input)
    assert pkg.xxh64_device(a.ctypes.data, len(data), 0, lib_path=emu_lib_path) == want


@pytest.mark.parametrize("n,off", LENGTH_CASES)
def test_lengths_and_alignments_emulator(pkg, O, emu_lib_path, n, off):
    buf = K.xxh64_input(n + off)
    a = buf[off:]
    for seed in K.XXH_SEEDS:
        assert pkg.xxh64_device(buf.ctypes.data + off, n, seed, lib_path=emu_lib_path) == _want(O, a, seed), (n, off, hex(seed))


@pytest.fixture(scope="module")
def gpu_buffer(graft):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    graft.build_hip()
    d = torch.from_numpy(K.xxh64_input(K.XXH_OFFSET_LEN + 16).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("n,off", LENGTH_CASES)
def test_lengths_and_alignments_gpu(pkg, O, gpu_buffer, n, off):
    a = K.xxh64_input(n + off)[off:]
    for seed in K.XXH_SEEDS:
        assert pkg.xxh64_device(gpu_buffer.data_ptr() + off, n, seed) == _want(O, a, seed), (n, off, hex(seed))


@pytest.mark.gpu
def test_known_answers_gpu(pkg, gpu_buffer):
    import torch
    d = torch.tensor(list(b"abc"), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert pkg.xxh64_device(d.data_ptr(), 0) == K.XXH_KNOWN[0][1]
    assert pkg.xxh64_device(d.data_ptr(), 3) == K.XXH_KNOWN[1][1]
