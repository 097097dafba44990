"""The plugin's LZMA2 decoder object (CGpuLzma2Decoder, row LZMA2GPU), driven the way a 7-Zip host drives a decoder (tests/host/plugin_host.cpp, unchanged).
CPU: the plugin layer over the emulator build; GPU (-m gpu): the product module lib7zgpucodec.so."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "_build")
BLK = 128 * 1024


def _host(module, *args):
    return subprocess.run([os.path.join(EMU, "plugin_host"), module] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def emu_module(emu_lib_path):
    return os.path.join(EMU, "lib7zgpucodec_emu.so")


def test_listing_has_a_decoder_only_row_at_the_end(emu_module):
    r = _host(emu_module, "list")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    last = lines[-1].split()
    assert last[0] == str(len(lines) - 1) and last[1:5] == ["21", "LZMA2GPU", "enc=0", "dec=1"]
    assert [l.split()[1:3] for l in lines[:3]] == [["4F71101", "ZSTD"], ["21", "FLZMA2"], ["4F71102", "BROTLI"]]       # the first rows as before
    assert "enc=1 dec=1" in lines[0] and "enc=1 dec=0" in lines[1] and "enc=1 dec=1" in lines[2]
    assert [l.split()[2] for l in lines].count("LZMA2GPU") == 1 and all("enc=1" in l for l in lines[:-1])
    # the row has no encoder: by index and by name
    r = _host(emu_module, "encode", "LZMA2GPU", 5, "/dev/null", "/dev/null")
    assert r.returncode == 8 and "method not found" in r.stderr


def _decode_cases(O, module, tmp_path, name, comp, prop, x):
    src, props = tmp_path / (name + ".lzma2"), tmp_path / (name + ".props")
    np.asarray(comp, dtype=np.uint8).tofile(src)
    props.write_bytes(bytes([prop]))
    for k, extra in enumerate(([], ["by-clsid"], ["size=%d" % x.size], ["by-clsid", "size=%d" % x.size])):
        dst = tmp_path / ("%s.%d.out" % (name, k))
        r = _host(module, "decode", "LZMA2GPU", props, src, dst, *extra)
        assert r.returncode == 0, r.stderr + r.stdout
        assert np.fromfile(dst, dtype=np.uint8).tobytes() == x.tobytes()
    for wrong in (x.size + 1, max(0, x.size - 1)):
        if wrong != x.size:
            r = _host(module, "decode", "LZMA2GPU", props, src, tmp_path / "wrong.out", "size=%d" % wrong)
            assert r.returncode == 15 and "80004005" in r.stderr, r.stderr + r.stdout      # E_FAIL


def _streams(O, pkg, lib_kw, n):
    x = O.corpus("silesia-like", n)
    enc = pkg.Flzma2Encoder(level=5, **lib_kw)
    try:
        own = np.concatenate([enc.code(x[:n // 2], flags=enc.NO_END_MARK), enc.code(x[n // 2:])])         # two units
        oprop = enc.coder_props()[0]
    finally:
        enc.close()
    out = [("own", own, oprop, x)]
    if O.ref("flzma2") is not None:
        ref, rprop = O.ref_fl2_compress(x, 5)
        out.append(("fl2", ref, rprop, x))
    return out


def test_decode_through_com_surface(O, pkg, emu_module, emu_lib_path, tmp_path):
    cases = _streams(O, pkg, dict(lib_path=emu_lib_path), BLK + 4321)
    assert len(cases) == 2 or O.ref("flzma2") is None
    for name, comp, prop, x in cases:
        _decode_cases(O, emu_module, tmp_path, name, comp, prop, x)
    # an empty stream, a damaged one, one without its end marker, bytes behind the end marker
    name, comp, prop, x = cases[0]
    _decode_cases(O, emu_module, tmp_path, "empty", np.zeros(1, dtype=np.uint8), prop, x[:0])
    props = tmp_path / "own.props"
    bad = comp.copy(); bad[comp.size // 2] ^= 0x10
    bad.tofile(tmp_path / "bad.lzma2")
    r = _host(emu_module, "decode", "LZMA2GPU", props, tmp_path / "bad.lzma2", tmp_path / "bad.out")
    assert r.returncode == 15 and "80004005" in r.stderr, r.stderr + r.stdout
    comp[:-1].tofile(tmp_path / "cut.lzma2")
    r = _host(emu_module, "decode", "LZMA2GPU", props, tmp_path / "cut.lzma2", tmp_path / "cut.out")
    assert r.returncode == 15 and "80004005" in r.stderr, r.stderr + r.stdout
    np.concatenate([comp, np.frombuffer(b"behind the end marker", dtype=np.uint8)]).tofile(tmp_path / "tail.lzma2")
    r = _host(emu_module, "decode", "LZMA2GPU", props, tmp_path / "tail.lzma2", tmp_path / "tail.out", "size=%d" % x.size)
    assert r.returncode == 0 and np.fromfile(tmp_path / "tail.out", dtype=np.uint8).tobytes() == x.tobytes(), r.stderr + r.stdout
    # a property blob that is not the one dictionary byte
    (tmp_path / "three.props").write_bytes(bytes([prop, 0, 0]))
    r = _host(emu_module, "decode", "LZMA2GPU", tmp_path / "three.props", tmp_path / "own.lzma2", tmp_path / "three.out")
    assert r.returncode == 12


def test_flzma2_rows_still_have_no_decoder(O, emu_module, tmp_path):
    x = O.corpus("text-zipf", 5000)
    src, dst, props = tmp_path / "in.bin", tmp_path / "out.lzma2", tmp_path / "props.bin"
    x.tofile(src)
    for name in ("FLZMA2", "FLZMA2GPU"):
        r = _host(emu_module, "encode", name, 5, src, dst, props)          # (plugin_host checks that CreateDecoder answers CLASS_E_CLASSNOTAVAILABLE for the row)
        assert r.returncode == 0, r.stderr + r.stdout
        r = _host(emu_module, "decode", name, props, dst, tmp_path / "no.out")
        assert r.returncode == 8
    r = _host(emu_module, "decode", "LZMA2GPU", props, dst, tmp_path / "yes.out", "size=%d" % x.size)
    assert r.returncode == 0 and np.fromfile(tmp_path / "yes.out", dtype=np.uint8).tobytes() == x.tobytes(), r.stderr + r.stdout


@pytest.mark.gpu
def test_product_plugin_lzma2_decoder_on_gpu(O, pkg, graft, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    graft.build_hip()
    module = graft.build_plugin()
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "emu"), "_build/plugin_host"], check=True, capture_output=True)
    r = _host(module, "list")
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].split()[1:5] == ["21", "LZMA2GPU", "enc=0", "dec=1"]
    for name, comp, prop, x in _streams(O, pkg, dict(device=0), 20 * 1024 * 1024 + 4321):
        _decode_cases(O, module, tmp_path, name, comp, prop, x)
