"""The batched zstd encoder (include/gpucodec.h "ZSTD, batched"; DESIGN.md section 4 "Batches"): item i of a batch compresses to exactly the bytes the stream call
writes for that item alone.  Cases and shared checks: tests/zstd_batch_cases.py; every test runs under the emulator and, marked gpu, on the device (through the
hooked test build, because some cases force small rounds with GC_BATCH_ROUND_ITEMS)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("zstd_batch_cases", os.path.join(HERE, "zstd_batch_cases.py"))
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def B(request):
    if request.param == "emu":
        return K.Backend("emu", dict(lib_path=request.getfixturevalue("emu_lib_path")))
    return K.Backend("gpu", request.getfixturevalue("gpu_hooks_kw"))


class Coders:
    """a batch encoder, a second encoder for the stream calls the contract compares against, a decoder"""
    def __init__(self, pkg, B, level=3):
        self.enc = pkg.ZstdEncoder(level=level, **B.kw)
        self.one = pkg.ZstdEncoder(level=level, **B.kw)
        self.dec = pkg.ZstdDecoder(**B.kw)

    def checksum(self, on):
        for e in (self.enc, self.one):
            e.set_option(e.OPT_ZSTD_CHECKSUM, 1 if on else 0)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.enc.close(); self.one.close(); self.dec.close()


def _run_and_check(B, O, cs, src, items, checksum=False):
    results, total, out, _ = K.run_batch(B, cs.enc, src, items)
    frames = K.check_batch(B, O, cs.one, cs.dec, src, items, results, total, out, checksum)
    return results, out, frames


# ------------------------------------------------------------------------------------------------ 1: sizes at every boundary the kernels have
def test_boundary_sizes(pkg, O, B):
    src, items = K.boundary_batch()
    with Coders(pkg, B) as cs:
        results, out, frames = _run_and_check(B, O, cs, src, items)
        assert frames[0].tobytes() == bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x00, 0x01, 0x00, 0x00])      # the empty item: the 9-byte empty frame
        # frame headers of 6, 7 and 9 bytes: the descriptor's Frame_Content_Size code is 0, 1, 2
        fcs = {n: frames[i][4] >> 6 for i, (_, n) in enumerate(items)}
        assert (fcs[255], fcs[256], fcs[65791], fcs[65792]) == (0, 1, 1, 2)
        # the host entry (gathered inputs, one copy each way) gives the same frames
        assert [f for f in cs.enc.code_batch([src[o:o + n] for o, n in items])] == [f.tobytes() for f in frames]


# ------------------------------------------------------------------------------------------------ 2: placement
def test_placement(pkg, O, B):
    src, items = K.placement_batch()
    with Coders(pkg, B) as cs:
        results, out, frames = _run_and_check(B, O, cs, src, items)
        assert frames[5].tobytes() == frames[6].tobytes()          # the item listed twice
        assert frames[7].tobytes() == frames[4].tobytes() and frames[11].tobytes() == frames[0].tobytes()      # ... and the ones listed again, in descending order


# ------------------------------------------------------------------------------------------------ 3: nothing leaks across an item's end
def test_nothing_leaks_across_an_items_end(pkg, O, B):
    src, items = K.leak_batch()
    with Coders(pkg, B) as cs:
        results, out, frames = _run_and_check(B, O, cs, src, items)
        assert frames[0].tobytes() == frames[1].tobytes() == frames[2].tobytes()      # identical items: no match reaches into the neighbour in front
        assert all(r.flags == 0 for r in results)


# ------------------------------------------------------------------------------------------------ 4: raw-block fallback and long matches
def test_raw_blocks_and_long_matches(pkg, O, B):
    src, items, raw = K.raw_batch()
    with Coders(pkg, B) as cs:
        results, out, frames = _run_and_check(B, O, cs, src, items)
        for i, ((o, n), r) in enumerate(zip(items, results)):
            assert (r.flags & 1) == (1 if i in raw else 0)
            if i in raw:
                hdr = 6 if n < 256 else (7 if n < 65536 + 256 else 9)
                assert r.dst_size == hdr + 3 + n and frames[i][hdr + 3:].tobytes() == src[o:o + n].tobytes()
        assert results[2].flags == 0                                 # 128 KiB of zeros: chains of capped matches, a compressed block


# ------------------------------------------------------------------------------------------------ 5: levels
@pytest.mark.parametrize("level", K.LEVELS)
def test_levels(pkg, O, B, level):
    src, items = K.level_batch()
    with Coders(pkg, B, level) as cs:
        _run_and_check(B, O, cs, src, items)


# ------------------------------------------------------------------------------------------------ 6: checksums
def test_checksums(pkg, O, B):
    src, items = K.boundary_batch()
    with Coders(pkg, B) as cs:
        cs.checksum(True)
        results, out, frames = _run_and_check(B, O, cs, src, items, checksum=True)
        K.check_checksums(O, src, items, frames)
        assert frames[0].size == 13
        cs.enc.set_option(cs.enc.OPT_ZSTD_SEEK_TABLE, 1)           # ignored by batch calls: `results` is the table
        r2, t2, out2, _ = K.run_batch(B, cs.enc, src, items)
        assert np.array_equal(out2, out) and [(r.dst_off, r.dst_size, r.flags) for r in r2] == [(r.dst_off, r.dst_size, r.flags) for r in results]
        cs.enc.set_option(cs.enc.OPT_ZSTD_SEEK_TABLE, 0)
        cs.checksum(False)
        _, plain, _ = _run_and_check(B, O, cs, src, items)          # the option off again: the bytes without checksums, those of the plain stream calls
        assert plain.size == out.size - 4 * len(items)


# ------------------------------------------------------------------------------------------------ 7: rounds
def test_rounds(pkg, O, B, monkeypatch):
    src, items = K.rounds_batch()
    with Coders(pkg, B) as cs:
        results, out, _ = _run_and_check(B, O, cs, src, items)
        table = [(r.dst_off, r.dst_size, r.flags) for r in results]
        for r in (3, 1):                                            # rounds of 3 + 3 + 2, then one item per round
            monkeypatch.setenv("GC_BATCH_ROUND_ITEMS", str(r))
            res, total, got, _ = K.run_batch(B, cs.enc, src, items)
            assert [(q.dst_off, q.dst_size, q.flags) for q in res] == table and np.array_equal(got, out), r
        cs.checksum(True)                                           # ... and with the checksum kernel's one launch beside the rounds
        monkeypatch.setenv("GC_BATCH_ROUND_ITEMS", "3")
        res, total, got, _ = K.run_batch(B, cs.enc, src, items)
        K.check_batch(B, O, cs.one, cs.dec, src, items, res, total, got, True)


# ------------------------------------------------------------------------------------------------ 8: refusals and edges
def test_refusals_and_edges(pkg, O, B):
    src, items = K.rounds_batch()
    big = np.concatenate([K.text(K.BLK), K.text(1000, 5)])         # 132072 bytes
    with Coders(pkg, B) as cs:
        enc = cs.enc
        d_src, p_src = B.upload(src)
        d_big, p_big = B.upload(big)
        cap = enc.batch_bound([n for _, n in items])
        d_dst, p_dst = B.filled(cap, 0xA5)
        # an item of one block + 1 byte: refused, with its index and size in the message
        assert K.raw_device_call(enc, pkg, p_big, big.size, [(0, 100), (7, K.BLK + 1)], p_dst, cap) == K.GC_ERR_PARAM
        assert "item 1" in K.last_error(enc) and str(K.BLK + 1) in K.last_error(enc)
        with pytest.raises(pkg.GpuCodecError, match="item 1"):
            enc.code_batch([big[:10], big[:K.BLK + 1]])
        # an item that ends behind srcBytes
        assert K.raw_device_call(enc, pkg, p_src, src.size, [(0, 100), (10, 20), (src.size - 99, 100)], p_dst, cap) == K.GC_ERR_PARAM
        assert "item 2" in K.last_error(enc)
        # finish without a pending batch (the refused calls above left none)
        assert K.raw_finish(enc, pkg, 0)[0] == K.GC_ERR_PARAM
        # nItems == 0
        assert K.raw_device_call(enc, pkg, p_src, src.size, [], p_dst, cap) == K.GC_OK
        assert K.raw_finish(enc, pkg, 0) == (K.GC_OK, 0)
        assert enc.code_batch([]) == []
        # a destination one byte short of the total: reported by finish, nothing written, and the context goes on working
        results, total, out, _ = K.run_batch(B, enc, src, items)
        assert K.raw_device_call(enc, pkg, p_src, src.size, items, p_dst, total - 1) == K.GC_OK
        rc, _ = K.raw_finish(enc, pkg, len(items))
        assert rc == K.GC_ERR_DST_SMALL and str(total) in K.last_error(enc)
        assert (B.download(d_dst, cap) == 0xA5).all()
        assert K.raw_finish(enc, pkg, len(items))[0] == K.GC_ERR_PARAM          # (that batch is finished)
        assert K.raw_device_call(enc, pkg, p_src, src.size, items, p_dst, total) == K.GC_OK      # exactly enough
        assert K.raw_finish(enc, pkg, len(items)) == (K.GC_OK, total)
        assert np.array_equal(B.download(d_dst, total), out) and (B.download(d_dst, cap)[total:] == 0xA5).all()
        # a stream call after a batch call and a batch call after a stream call, on one context
        x = np.concatenate([K.text(3 * K.BLK + 77, 9)])
        assert np.array_equal(cs.dec.code(enc.code(x)), x) and np.array_equal(enc.code(x), cs.one.code(x))
        r2, t2, out2, _ = K.run_batch(B, enc, src, items)
        K.check_batch(B, O, cs.one, cs.dec, src, items, r2, t2, out2)
        assert np.array_equal(enc.code(src[:5000]), cs.one.code(src[:5000]))
        # timing of the last batch call
        ms = enc.batch_timing_ms()
        assert set(ms) == set(enc.BATCH_KERNELS) and all(v >= 0.0 for v in ms.values())
        assert enc.batch_round_items() >= 4 * 256                   # a round fills the device several times over at one K1b workgroup per CU


# ------------------------------------------------------------------------------------------------ 9: GPU only -- more items than CUs
@pytest.mark.gpu
def test_more_items_than_compute_units(pkg, O, gpu_hooks_kw, monkeypatch):
    import torch
    B = K.Backend("gpu", gpu_hooks_kw)
    src, items = K.many_batch()
    monkeypatch.setenv("GC_BATCH_ROUND_ITEMS", str(K.MANY_ROUND_ITEMS))      # three rounds
    with Coders(pkg, B) as cs:
        d_src, p_src = B.upload(src)
        cap = cs.enc.batch_bound([n for _, n in items])
        d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        cs.enc.code_batch_device(p_src, src.size, items, d_dst.data_ptr(), cap)
        results, total = cs.enc.finish_batch(len(items))
        ms = cs.enc.batch_timing_ms()
        print("600 items, %d -> %d bytes, timing %s" % (sum(n for _, n in items), total, ms))
        assert all(v > 0.0 for v in ms.values())
        K.check_layout(items, results, total)
        out = d_dst[:total].cpu().numpy()
        # (a) on the first, the last and 30 seeded items
        spot = [0, len(items) - 1] + [int(i) for i in np.random.default_rng(30).choice(len(items), K.MANY_SPOT, replace=False)]
        for i in spot:
            o, n = items[i]
            r = results[i]
            assert out[r.dst_off:r.dst_off + r.dst_size].tobytes() == K.single_call(B, cs.one, src[o:o + n], False), i
        # (b) the whole output under the oracle's decoder (and the reference's)
        content = np.concatenate([src[o:o + n] for o, n in items])
        assert np.array_equal(O.port_zstd_decompress(out, content.size), content)
        if O.ref("zstd") is not None:
            assert np.array_equal(O.ref_zstd_decompress(out, content.size), content)
        # (c) through the device decoder, the content compared where it lies
        frames, nf, stated = cs.dec.scan(out)
        assert nf == len(items) and stated == content.size
        d_out = torch.empty(content.size + 64, dtype=torch.uint8, device="cuda:0")
        got = cs.dec.code_device(d_dst.data_ptr(), total, d_out.data_ptr(), content.size, frames, nf)
        want = torch.cat([d_src[o:o + n] for o, n in items])
        assert got == content.size and torch.equal(d_out[:content.size], want)
        assert [frames[i].content_size for i in range(nf)] == [n for _, n in items]      # ... which, cut at the frames' content sizes, is the items
