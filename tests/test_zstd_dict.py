"""Raw-content zstd dictionaries for the batch encoder and the decoder (include/gpucodec.h "ZSTD, dictionaries"; DESIGN.md section 4 "Dictionaries").  Cases, the
records generator, the reference's dictionary calls and the model of hand-built frames: tests/zstd_dict_cases.py.  Every test runs under the emulator and, marked
gpu, on the device (through the hooked test build: the cases force execution paths and round sizes with GC_* hooks).  The interoperability cases need the
reference library (oracle/_ref/libzstd_ref.so, made by build()); without it they skip."""
import importlib.util
import os
import struct

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("zstd_dict_cases", os.path.join(HERE, "zstd_dict_cases.py"))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)
K, Z = D.K, D.Z

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def B(request):
    if request.param == "emu":
        return K.Backend("emu", dict(lib_path=request.getfixturevalue("emu_lib_path")))
    return K.Backend("gpu", request.getfixturevalue("gpu_hooks_kw"))


@pytest.fixture(scope="module")
def ref(O):
    if O.ref("zstd") is None:
        pytest.skip("the reference library is not built")
    return D.Ref(O.ref("zstd"))


def decode_both_paths(dec, frames, items, monkeypatch, seqv=(None,)):
    """ZstdDecoder.code_batch gives the items back on the frame-per-workgroup path and on the wide path (and with either sequences kernel)"""
    for wide in ("0", "1"):
        monkeypatch.setenv("GC_ZD_WIDE", wide)
        for sv in seqv:
            if sv is not None:
                monkeypatch.setenv("GC_ZD_SEQV", sv)
            got = dec.code_batch(frames)
            assert len(got) == len(items)
            for i, (g, x) in enumerate(zip(got, items)):
                assert np.array_equal(g, x), (wide, sv, i)
    monkeypatch.delenv("GC_ZD_WIDE")
    monkeypatch.delenv("GC_ZD_SEQV", raising=False)


def batch(B, enc, parts):
    src, items = K.packed(parts)
    results, total, out, _ = K.run_batch(B, enc, src, items)
    K.check_layout(items, results, total)
    return D.frames_of(out, results), results, total


# ------------------------------------------------------------------------------------------------ 1: dictionary sizes x item sizes
@pytest.mark.parametrize("ds", D.DICT_SIZES)
def test_dictionary_and_item_sizes(pkg, ref, B, monkeypatch, ds):
    d, parts, frames, results, total, items = D.sweep_total(pkg, B, ds)
    K.check_layout(items, results, total)
    for f, x in zip(frames, parts):
        y = ref.decompress(f, d, x.size)
        assert y is not None and np.array_equal(y, x), x.size
    dec = pkg.ZstdDecoder(**B.kw)
    try:
        dec.set_dictionary(d)
        assert dec.dictionary_size() == ds
        decode_both_paths(dec, frames, parts, monkeypatch)
    finally:
        dec.close()
    assert total == D.golden_sizes()["sweep"][str(ds)]              # the recorded total of the emulator run: a device-only divergence shows as a size


# ------------------------------------------------------------------------------------------------ 2: constructed items
def test_item_is_the_dictionarys_tail(pkg, ref, B, monkeypatch):
    d = D.record_dict(16 << 10)
    x = d[-3000:]
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        (f,), (r,), _ = batch(B, enc, [x])
        assert len(f) < 60 and r.flags == 0
        assert D.walk_offsets(f) == [(0, 3000, 3000)]
        assert np.array_equal(ref.decompress(f, d, x.size), x)
        assert ref.decompress(f, None, x.size) is None               # without the dictionary the reference refuses the frame
        decode_both_paths(dec, [f], [x], monkeypatch)
    finally:
        enc.close(); dec.close()


def test_match_that_would_run_over_the_dictionarys_end(pkg, ref, B, monkeypatch):
    a, b = K.text(5000, 100), D.records(700, 77)
    d, x = np.concatenate([a, b]), np.concatenate([b, b])
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        (f,), (r,), _ = batch(B, enc, [x])
        assert r.flags == 0 and len(f) < 60                           # B from the dictionary's end, B again from the dictionary or the item: a few sequences
        assert np.array_equal(ref.decompress(f, d, x.size), x)
        decode_both_paths(dec, [f], [x], monkeypatch)
    finally:
        enc.close(); dec.close()


def test_item_is_the_whole_largest_dictionary(pkg, ref, B, monkeypatch):
    d = D.mixed_dict(D.DICT_MAX)
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        (f,), (r,), _ = batch(B, enc, [d])
        assert r.flags == 0 and len(f) < 64                           # compressed, not raw: the chain of 2048 capped matches at offset 128 KiB merges
        assert D.walk_offsets(f) == [(0, D.DICT_MAX, D.DICT_MAX)]        # ... into one sequence
        assert np.array_equal(ref.decompress(f, d, d.size), d)
        decode_both_paths(dec, [f], [d], monkeypatch)
    finally:
        enc.close(); dec.close()


def test_largest_offset(pkg, ref, B, monkeypatch):
    """Bytes [-300, -100) of a 128 KiB item are the first 200 bytes of a 128 KiB dictionary: a match there has offset position + dictSize - dictionary position, above
    260 000, the largest the feature can produce.  Walking the frame's sequences with the model's repeat offsets shows it; and with another dictionary that differs in
    exactly those 200 bytes both decoders regenerate an item that differs from the right one in [-300, -100) only."""
    d = np.array(D.mixed_dict(D.DICT_MAX))
    d[:200] = K.rand(200, 9)                                           # (found nowhere else)
    x = np.array(K.rand(D.BLK, 10))
    x[:D.BLK - 400] = np.resize(D.records(30000, 55), D.BLK - 400)
    x[-300:-100] = d[:200]
    d2 = d.copy(); d2[:200] ^= 0xFF
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        (f,), (r,), _ = batch(B, enc, [x])
        assert r.flags == 0
        far = [(pos, ml, off) for pos, ml, off in D.walk_offsets(f) if off > 260000]
        assert far and all(D.BLK - 300 <= pos and pos + ml <= D.BLK - 100 and off == pos + D.DICT_MAX - (pos - (D.BLK - 300)) for pos, ml, off in far), far
        assert np.array_equal(ref.decompress(f, d, x.size), x)
        decode_both_paths(dec, [f], [x], monkeypatch)
        y = ref.decompress(f, d2, x.size)
        outside = np.r_[0:D.BLK - 300, D.BLK - 100:D.BLK]
        assert y is not None and np.array_equal(y[outside], x[outside]) and not np.array_equal(y, x)      # bytes of [-300, -100), and no others, come from dictionary[0:200]
        dec.set_dictionary(d2)
        assert np.array_equal(dec.code(f), y)
    finally:
        enc.close(); dec.close()


def test_random_item_and_identical_items(pkg, ref, B, monkeypatch):
    d = D.record_dict(16 << 10)
    same, noise = D.records(2000, 31), K.rand(3000, 4)
    parts = [same, noise, D.records(500, 32), same, K.text(900, 5), same]
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        frames, results, _ = batch(B, enc, parts)
        assert results[1].flags == 1 and frames[1][-3000:] == noise.tobytes()      # a raw block
        assert frames[0] == frames[3] == frames[5]
        for f, x in zip(frames, parts):
            assert np.array_equal(ref.decompress(f, d, x.size), x)
        decode_both_paths(dec, frames, parts, monkeypatch)
    finally:
        enc.close(); dec.close()


# ------------------------------------------------------------------------------------------------ 3: determinism
def test_determinism_and_round_sizes(pkg, B, monkeypatch):
    d, parts = D.record_dict(16 << 10), D.record_items(8, 700) + [D.records(0, 1), K.text(5000, 3)]
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        frames, results, total = batch(B, enc, parts)
        again, _, _ = batch(B, enc, parts)
        assert again == frames
        for r in (3, 1):
            monkeypatch.setenv("GC_BATCH_ROUND_ITEMS", str(r))
            got, res, tot = batch(B, enc, parts)
            assert got == frames and tot == total, r
        monkeypatch.delenv("GC_BATCH_ROUND_ITEMS")
        assert enc.code_batch(parts) == frames                        # the host entry
    finally:
        enc.close(); dec.close()


# ------------------------------------------------------------------------------------------------ 4: checksums
def test_checksums_cover_the_item_alone(pkg, O, ref, B, monkeypatch):
    d, parts = D.record_dict(16 << 10), D.record_items(6, 900) + [D.records(0, 1)]
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        enc.set_option(enc.OPT_ZSTD_CHECKSUM, 1)
        frames, results, _ = batch(B, enc, parts)
        for f, x in zip(frames, parts):
            assert f[4] & 4 and struct.unpack("<I", f[-4:])[0] == K.xxh32(O, x) == Z.xxh64(x.tobytes()) & 0xFFFFFFFF
            assert np.array_equal(ref.decompress(f, d, x.size), x)    # libzstd verifies the checksum
        decode_both_paths(dec, frames, parts, monkeypatch)
        # a dictionary that differs in one byte the first frame uses: the content comes out different, the checksum says so
        used = None
        for p in range(d.size - 1, -1, -1):
            d2 = d.copy(); d2[p] ^= 0x55
            y = ref.decompress(frames[0], d2, parts[0].size)
            if y is None:
                used = p
                break
        assert used is not None
        d2 = d.copy(); d2[used] ^= 0x55
        dec.set_dictionary(d2)
        for wide in ("0", "1"):
            monkeypatch.setenv("GC_ZD_WIDE", wide)
            rc, _ = D.raw_decode(dec, frames[0], parts[0].size)
            assert rc == D.GC_ERR_CORRUPT, wide
        monkeypatch.delenv("GC_ZD_WIDE")
        dec.set_dictionary(d)
        assert np.array_equal(dec.code(frames[0]), parts[0])          # the context goes on working
    finally:
        enc.close(); dec.close()


# ------------------------------------------------------------------------------------------------ 5: levels
@pytest.mark.parametrize("level", D.LEVELS)
def test_levels(pkg, ref, B, monkeypatch, level):
    d, parts = D.record_dict(16 << 10), D.record_items(8, 1500)
    enc, dec = D.dict_coders(pkg, B, d, level)
    try:
        frames, _, _ = batch(B, enc, parts)
        for f, x in zip(frames, parts):
            assert np.array_equal(ref.decompress(f, d, x.size), x)
        decode_both_paths(dec, frames, parts, monkeypatch)
    finally:
        enc.close(); dec.close()


# ------------------------------------------------------------------------------------------------ 6: switching off and refusals
def test_switching_off_and_refusals(pkg, B):
    d, parts = D.record_dict(16 << 10), D.record_items(6, 800)
    enc, dec = D.dict_coders(pkg, B, None)
    fresh = pkg.ZstdEncoder(level=3, **B.kw)
    try:
        today = fresh.code_batch(parts)
        assert enc.dictionary_size() == 0
        enc.set_dictionary(d)
        assert enc.dictionary_size() == d.size
        withd = enc.code_batch(parts)
        assert withd != today and sum(map(len, withd)) < sum(map(len, today))
        # the refusals; after each the dictionary in place is still there and the context goes on working
        for bad, rc, word in [(d[:n].tobytes(), D.GC_ERR_PARAM, "fewer than 8") for n in range(1, 8)] + [
                (bytes(D.DICT_MAX + 1), D.GC_ERR_PARAM, "GC_ZSTD_DICT_MAX"),
                (struct.pack("<I", D.DICT_MAGIC) + d[:500].tobytes(), D.GC_ERR_UNSUPPORTED, "formatted")]:
            for coder in (enc, dec):
                assert D.raw_set_dictionary(coder, bad) == rc and word in D.last_error(coder), (len(bad), word)
            assert enc.dictionary_size() == d.size
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_UNSUPPORTED"):
            enc.set_dictionary(struct.pack("<I", D.DICT_MAGIC) + bytes(100))
        assert enc.code_batch(parts) == withd
        # the stream calls on a context that holds a dictionary are refused, never silently dictionary-less
        with pytest.raises(pkg.GpuCodecError, match="GC_ERR_UNSUPPORTED.*dictionary"):
            enc.code(parts[0])
        d_src, p_src = B.upload(parts[0])
        d_dst, p_dst = B.filled(4096, 0)
        assert enc._lib.gc_zstd_compress_device(enc._ctx, p_src, parts[0].size, p_dst, 4096, 3) == D.GC_ERR_UNSUPPORTED
        assert enc.code_batch(parts) == withd
        # set_dictionary between code_batch_device and finish_batch: the pending batch is whole and was coded with the old dictionary
        src, items = K.packed(parts)
        d_src, p_src = B.upload(src)
        cap = enc.batch_bound([n for _, n in items])
        d_dst, p_dst = B.filled(cap, 0xA5)
        enc.code_batch_device(p_src, src.size, items, p_dst, cap)
        enc.set_dictionary(D.record_dict(4096, 5))
        results, total = enc.finish_batch(len(items))
        assert D.frames_of(B.download(d_dst, total), results) == withd
        assert enc.code_batch(parts) != withd                         # ... and the next one with the new
        # switching off restores today's bytes exactly
        enc.set_dictionary(None)
        assert enc.dictionary_size() == 0 and enc.code_batch(parts) == today
        assert np.array_equal(enc.code(parts[0]), fresh.code(parts[0]))
    finally:
        enc.close(); dec.close(); fresh.close()


# ------------------------------------------------------------------------------------------------ 7: GPU only -- more items than CUs, three rounds
@pytest.mark.gpu
def test_more_items_than_compute_units(pkg, ref, gpu_hooks_kw, monkeypatch):
    import torch
    B = K.Backend("gpu", gpu_hooks_kw)
    src, items = D.many_batch()
    d = D.mixed_dict(D.MANY_DICT)
    monkeypatch.setenv("GC_BATCH_ROUND_ITEMS", str(D.MANY_ROUND_ITEMS))
    enc, dec = D.dict_coders(pkg, B, d)
    try:
        d_src, p_src = B.upload(src)
        cap = enc.batch_bound([n for _, n in items])
        d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        enc.code_batch_device(p_src, src.size, items, d_dst.data_ptr(), cap)
        results, total = enc.finish_batch(len(items))
        print("600 items, %d -> %d bytes, timing %s" % (src.size, total, enc.batch_timing_ms()))
        K.check_layout(items, results, total)
        out = d_dst[:total].cpu().numpy()
        for i in [int(i) for i in np.random.default_rng(32).choice(len(items), D.MANY_SPOT, replace=False)]:
            (o, n), r = items[i], results[i]
            assert np.array_equal(ref.decompress(out[r.dst_off:r.dst_off + r.dst_size], d, n), src[o:o + n]), i
        frames, nf, stated = dec.scan(out)
        assert nf == len(items) and stated == src.size
        d_out = torch.empty(src.size + 64, dtype=torch.uint8, device="cuda:0")
        got = dec.code_device(d_dst.data_ptr(), total, d_out.data_ptr(), src.size, frames, nf)
        assert got == src.size and torch.equal(d_out[:src.size], d_src)
    finally:
        enc.close(); dec.close()


# ------------------------------------------------------------------------------------------------ 8: frames of the reference's encoder
@pytest.mark.parametrize("level", D.REF_LEVELS)
def test_reference_encoder_frames(pkg, ref, B, monkeypatch, level):
    d = D.record_dict(16 << 10)
    parts = D.record_items(8, 300) + D.record_items(4, 4096, 6)
    frames = [ref.compress(x, d, level) for x in parts]
    dec = pkg.ZstdDecoder(**B.kw)
    try:
        dec.set_dictionary(d)
        decode_both_paths(dec, frames, parts, monkeypatch, seqv=("0", "1"))
        # one input of three blocks behind a 64 KiB dictionary: later blocks reach the dictionary across block borders and through carried repeat offsets
        d64 = D.record_dict(64 << 10, 8)
        big = np.concatenate([d64[5000:60000], D.records(300 * 1024 - 55000 - 40000, 9), d64[20000:60000]])
        f = ref.compress(big, d64, level)
        assert ref.decompress(f, None, big.size) is None              # (it does reach the dictionary)
        dec.set_dictionary(d64)
        decode_both_paths(dec, [f], [big], monkeypatch, seqv=("0", "1"))
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ 9, 10, 11: hand-built frames
def test_handmade_frames(pkg, ref, B, monkeypatch):
    d = D.record_dict(777, 12).tobytes()
    frames = D.handmade(d)
    assert set(frames) >= {"ll0_rep", "span", "first_byte", "past_first_bad", "raw_rle_then", "second_block_rep", "no_reach"}
    dec, plain = pkg.ZstdDecoder(**B.kw), pkg.ZstdDecoder(**B.kw)
    try:
        dec.set_dictionary(d)
        for name, f in frames.items():
            data, want = f.bytes(single=True), np.frombuffer(f.content, dtype=np.uint8)
            assert f.sound == (not name.endswith("_bad")), name
            theirs = ref.decompress(data, d, len(want) + 64)
            assert (theirs is not None) == f.sound, name               # accepted by one means accepted by both
            theirs_plain = ref.decompress(data, None, len(want) + 64)
            assert (theirs_plain is not None) == (name == "no_reach"), name
            for wide in ("0", "1"):
                monkeypatch.setenv("GC_ZD_WIDE", wide)
                for sv in ("0", "1"):
                    monkeypatch.setenv("GC_ZD_SEQV", sv)
                    rc, got = D.raw_decode(dec, data, len(want))
                    if f.sound:
                        assert rc == D.GC_OK and np.array_equal(got, want) and np.array_equal(theirs, want), (name, wide, sv)
                    else:
                        assert rc == D.GC_ERR_CORRUPT, (name, wide, sv)
                    # the same frame with no dictionary set keeps today's verdict
                    rc, got = D.raw_decode(plain, data, len(want))
                    if name == "no_reach":
                        assert rc == D.GC_OK and np.array_equal(got, want), (name, wide, sv)      # 11: ... and decodes the same with and without
                    else:
                        assert rc == D.GC_ERR_CORRUPT, (name, wide, sv)
        monkeypatch.delenv("GC_ZD_WIDE"); monkeypatch.delenv("GC_ZD_SEQV")
        # 10: a nonzero dictionary id while a dictionary is set
        f = frames["no_reach"]
        rc, _ = D.raw_decode(dec, f.bytes(single=True, did=5, did_bytes=1), len(f.content))
        assert rc == D.GC_ERR_PARAM
        assert ref.decompress(f.bytes(single=True, did=5, did_bytes=1), d, 4096) is None      # (the reference: dictionary_wrong)
        # 11: a no-dictionary frame of this engine through a context with a dictionary
        x = K.text(3 * D.BLK + 99, 50)
        enc = pkg.ZstdEncoder(level=3, **B.kw)
        try:
            assert np.array_equal(dec.code(enc.code(x)), x)
        finally:
            enc.close()
    finally:
        dec.close(); plain.close()


# ------------------------------------------------------------------------------------------------ size
@pytest.mark.parametrize("name", sorted(D.SIZE_BATCHES))
def test_size_against_the_reference(pkg, ref, B, name):
    """R0 = engine / reference (level 3) without the dictionary, R1 with it; the bar is R1 <= max(R0, 1.0) + 0.02 (the project's parity band over the ratio of the
    path the dictionary path extends), and the dictionary must make the engine's total smaller.  Figures: profiles/zstd_dict.md."""
    d, items = D.size_batch(name)
    m = {}
    enc = pkg.ZstdEncoder(level=3, **B.kw)
    try:
        m["engine_plain"] = sum(map(len, enc.code_batch(items)))
        enc.set_dictionary(d)
        m["engine_dict"] = sum(map(len, enc.code_batch(items)))
    finally:
        enc.close()
    m["ref_plain"] = sum(len(ref.compress(x, None, 3)) for x in items)
    m["ref_dict"] = sum(len(ref.compress(x, d, 3)) for x in items)
    r0, r1 = m["engine_plain"] / m["ref_plain"], m["engine_dict"] / m["ref_dict"]
    print("%s: %s R0 %.4f R1 %.4f" % (name, m, r0, r1))
    assert m["ref_dict"] <= 0.75 * m["ref_plain"]                     # the batch is one on which the reference alone gains at least 25 %
    assert m["engine_dict"] < m["engine_plain"]
    assert r1 <= max(r0, 1.0) + 0.02
    assert m == D.golden_sizes()[name]                                # the recorded totals (emulator run): the device gives the same
