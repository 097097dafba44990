"""GC_OPT_ZSTD_CHECKSUM / GC_ZSTD_CHECKSUM: every zstd frame ends with the low 32 bits of XXH64 of its content, hashed on the device (what the
reference's bare-file handler writes, CPP/7zip/Archive/ZstdHandler.cpp:276).  Cases and shared checks: tests/zstd_checksum_cases.py; the emulator and the
device run the same ones."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("zstd_checksum_cases", os.path.join(HERE, "zstd_checksum_cases.py"))
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)

CASES = sorted(K.stream_cases(), key=lambda c: -c[2] * (4 if c[0] >= 16 else 1))       # the longest first (worker processes)
UNHOOKED_EMU = (3, "text-zipf", 3 * K.BLK + 77, False)      # the level's own 8 MiB frames: one frame here
UNHOOKED_GPU = (3, "text-zipf", 20_000_000, False)          # three 8 MiB frames, the last one short
GC_ERR_PARAM = -5


def _run_case(pkg, O, monkeypatch, case, **kw):
    if case[3]:
        monkeypatch.setenv("GC_FRAME_BLOCKS", str(K.HOOK_FRAME_BLOCKS))
    enc = pkg.ZstdEncoder(level=case[0], **kw)
    dec = pkg.ZstdDecoder(**{k: v for k, v in kw.items() if k != "level"})
    try:
        streams = K.encode_all(enc, K.case_input(case))
        K.check_case(O, dec, case, streams)
    finally:
        enc.close(); dec.close()
    return streams


def _refusals(pkg, O, dec, c, n):
    """who refuses the stream: (reference decoder, oracle restatement, the engine's decoder)"""
    out = []
    for f in (lambda: O.ref_zstd_decompress(c, n), lambda: O.port_zstd_decompress(c, n)):
        try:
            f(); out.append(False)
        except ValueError:
            out.append(True)
    try:
        dec.code(c); out.append(False)
    except pkg.GpuCodecError as e:
        assert "GC_ERR_CORRUPT" in str(e)
        out.append(True)
    return tuple(out)


def _damage(pkg, O, monkeypatch, **kw):
    case = K.DAMAGE_CASE
    monkeypatch.setenv("GC_FRAME_BLOCKS", str(K.HOOK_FRAME_BLOCKS))
    x = K.case_input(case)
    enc = pkg.ZstdEncoder(level=case[0], **kw); dec = pkg.ZstdDecoder(**kw)
    try:
        enc.set_option(enc.OPT_ZSTD_CHECKSUM, 1)
        c = enc.code(x).copy()
        assert _refusals(pkg, O, dec, c, x.size) == (False, False, False)
        frames, nf, _ = dec.scan(c)
        assert nf == 2
        bad = c.copy()
        bad[frames[1].src_off + frames[1].src_size - 3] ^= 0x10              # one bit of the second frame's checksum
        assert _refusals(pkg, O, dec, bad, x.size) == (True, True, True)
    finally:
        enc.close(); dec.close()


def _host_call(pkg, enc, x, flags):
    cap = enc.compress_bound(x.size)
    out = np.empty(cap, dtype=np.uint8); n = C.c_size_t(0)
    rc = enc._lib.gc_codec_compress_host(enc._ctx, pkg.CODEC_ZSTD, x.ctypes.data, x.size, out.ctypes.data, cap, enc.level, flags, C.byref(n))
    assert rc == pkg.GC_OK
    return out[:n.value].copy()


def _per_call_flag(pkg, monkeypatch, **kw):
    case = K.DAMAGE_CASE
    monkeypatch.setenv("GC_FRAME_BLOCKS", str(K.HOOK_FRAME_BLOCKS))
    x = K.case_input(case)
    enc = pkg.ZstdEncoder(level=case[0], **kw)
    try:
        s = K.encode_all(enc, x)
        ms = C.c_float(0)
        assert enc._lib.gc_zstd_checksum_timing(enc._ctx, C.byref(ms)) == GC_ERR_PARAM and enc.checksum_ms() is None     # the last call was a plain one
        assert np.array_equal(_host_call(pkg, enc, x, enc.CHECKSUM), s["sum"])                                        # flag on a context without the option
        assert enc._lib.gc_zstd_checksum_timing(enc._ctx, C.byref(ms)) == pkg.GC_OK and enc.checksum_ms() >= 0.0
        assert np.array_equal(_host_call(pkg, enc, x, 0), s["plain"])                                                 # ... and plain bytes again
        assert enc.checksum_ms() is None
    finally:
        enc.close()


def _multi(pkg, O, monkeypatch, **kw):
    monkeypatch.setenv("GC_FRAME_BLOCKS", str(K.HOOK_FRAME_BLOCKS))
    piece = K.HOOK_FRAME_BLOCKS * K.BLK
    x = K.case_input((3, "text-zipf", 2 * piece + 4321, True))               # three pieces of one frame each
    m = pkg.MultiEncoder("zstd", 3, **kw)
    dec = pkg.ZstdDecoder(**{k: v for k, v in kw.items() if k == "lib_path"})
    try:
        c = m.code(x, flags=8, piece_bytes=piece).copy()
        plain = m.code(x, piece_bytes=piece).copy()
        K.decodes_everywhere(O, dec, c, x)
        walked = K.walk_checksummed(O, dec, c, x, 3)
        assert np.array_equal(K.strip_checksums(c, walked), plain)
    finally:
        m.close(); dec.close()


# ------------------------------------------------------------------------------------------------ emulator
@pytest.mark.parametrize("case", CASES + [UNHOOKED_EMU], ids=K.case_id)
def test_checksummed_streams_emulator(pkg, O, emu_lib_path, monkeypatch, case):
    _run_case(pkg, O, monkeypatch, case, lib_path=emu_lib_path)


def test_damaged_checksum_is_refused_by_all_decoders_emulator(pkg, O, emu_lib_path, monkeypatch):
    _damage(pkg, O, monkeypatch, lib_path=emu_lib_path)


def test_per_call_flag_and_timing_emulator(pkg, emu_lib_path, monkeypatch):
    _per_call_flag(pkg, monkeypatch, lib_path=emu_lib_path)


def test_multi_hands_the_flag_to_every_piece_emulator(pkg, O, emu_lib_path, monkeypatch):
    monkeypatch.setenv("HIPEMU_DEVICES", "2")
    _multi(pkg, O, monkeypatch, lib_path=emu_lib_path)


# ------------------------------------------------------------------------------------------------ device
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=K.case_id)
def test_checksummed_streams_gpu(pkg, O, gpu_hooks_kw, monkeypatch, case):
    _run_case(pkg, O, monkeypatch, case, **gpu_hooks_kw)


@pytest.mark.gpu
def test_checksummed_stream_of_8_mib_frames_gpu(pkg, O, gpu_enc, monkeypatch):
    assert K.n_frames(UNHOOKED_GPU) == 3
    _run_case(pkg, O, monkeypatch, UNHOOKED_GPU, device=0)                   # the shipped library: no hooks


@pytest.mark.gpu
def test_damaged_checksum_is_refused_by_all_decoders_gpu(pkg, O, gpu_hooks_kw, monkeypatch):
    _damage(pkg, O, monkeypatch, **gpu_hooks_kw)


@pytest.mark.gpu
def test_per_call_flag_and_timing_gpu(pkg, gpu_hooks_kw, monkeypatch):
    _per_call_flag(pkg, monkeypatch, **gpu_hooks_kw)


@pytest.mark.gpu
def test_multi_hands_the_flag_to_every_piece_gpu(pkg, O, gpu_hooks_kw, monkeypatch):
    _multi(pkg, O, monkeypatch, lib_path=gpu_hooks_kw["lib_path"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", K.PARITY_CASES, ids=K.case_id)
def test_device_bytes_equal_emulator_bytes(pkg, gpu_hooks_kw, emu_lib_path, monkeypatch, case):
    monkeypatch.setenv("GC_FRAME_BLOCKS", str(K.HOOK_FRAME_BLOCKS))
    x = K.case_input(case)
    got = {}
    for name, kw in (("gpu", gpu_hooks_kw), ("emu", dict(lib_path=emu_lib_path))):
        enc = pkg.ZstdEncoder(level=case[0], **kw)
        try:
            enc.set_option(enc.OPT_ZSTD_CHECKSUM, 1); enc.set_option(enc.OPT_ZSTD_SEEK_TABLE, 1)
            got[name] = enc.code(x).copy()
        finally:
            enc.close()
    assert np.array_equal(got["gpu"], got["emu"])
