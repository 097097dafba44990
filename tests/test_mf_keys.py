"""Which positions the windowed finder lists, and with which keys (csrc/gc_lz_window.hip: mf_list, mf_listed, mf_window, mf_keys), is decided in one place that W1
(count), W3 (scatter, twice per position) and W5 (the unlisted positions) share.  How that place computes -- tile-relative limits, windows from aligned words and
funnel shifts, entries packed in halves -- must not move one compressed byte and not one list entry.

  * Streams: every case of tests/mf_keys_cases.py (planted byte runs at tile, block and frame edges; frame ends at every tile offset that matters; odd tile tails; a
    second frame too short to list anything) compresses to the SHA-256 that tools/record_mf_keys.py recorded from the emulator build of the commit named in
    tests/golden/mf_keys_sha256.json (`_parent_commit`), under frames of two blocks (test hook GC_FRAME_BLOCKS).  Emulator and device (-m gpu) against the same entries.
  * Lists: the test entry gc_test_mf_lists runs W1..W3 alone; the offsets table and the entry array must equal a numpy model of the predicate and of the base and far
    keys, in both geometries: counts per (tile, partition) -- that is W1 --, every entry in its place and positions ascending inside every run -- that is W3."""
import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mf_keys_sha256.json")

_spec = importlib.util.spec_from_file_location("mf_keys_cases", os.path.join(HERE, "mf_keys_cases.py"))
K = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K)

CASES = K.cases()


@pytest.fixture(scope="module")
def golden():
    d = json.load(open(GOLDEN))
    assert len(d["_parent_commit"]) == 40
    return d["sha256"]


@pytest.fixture(scope="module")
def inputs():
    """every input once per module: (name, tile) -> bytes"""
    cache = {}
    def get(name, tile):
        if (name, tile) not in cache:
            cache[(name, tile)] = K.build(name, tile)
            cache[(name, tile)].setflags(write=False)
        return cache[(name, tile)]
    return get


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(K.case_id(c) for c in CASES)


def test_inputs_hold_what_they_are_for():
    """the planted structure is there: runs at a frame's first byte and across tile edges of both geometries, sizes that put frame end - 80 where the names say"""
    for tile in (8192, 16384):
        x = K.build("runs", tile)
        assert x.size <= 5 * K.BLK and x[K.FRAME - 1] == x[K.FRAME] == x[K.FRAME + 7] and x[2 * K.FRAME] == x[2 * K.FRAME + 11] != x[2 * K.FRAME - 1]
        assert any(len(set(x[e - 1:e + 8].tolist())) == 1 for e in range(tile, 2 * K.FRAME, tile))
        for k in K.END_KS:
            assert K.build("end+%d" % k, tile).size - K.FRAME - K.WINDOW == k - 80 and K.build("endtile+%d" % k, tile).size - K.FRAME - tile - K.WINDOW == k - 80
        for k in K.TAIL_KS:
            assert K.build("tail+%d" % k, tile).size % tile == k


@pytest.mark.parametrize("case", CASES, ids=K.case_id)
def test_emulator_stream_unchanged(pkg, emu_lib_path, golden, monkeypatch, case):
    monkeypatch.setenv("GC_FRAME_BLOCKS", str(K.FRAME_BLOCKS))
    assert K.stream_sha256(pkg, case, lib_path=emu_lib_path) == golden[K.case_id(case)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=K.case_id)
def test_gpu_stream_unchanged(pkg, gpu_hooks_kw, golden, monkeypatch, case):
    monkeypatch.setenv("GC_FRAME_BLOCKS", str(K.FRAME_BLOCKS))
    assert K.stream_sha256(pkg, case, **gpu_hooks_kw) == golden[K.case_id(case)]


# ---------------------------------------------------------------------------------------------------- the lists against the model
@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def enc(request, pkg):
    kw = dict(lib_path=request.getfixturevalue("emu_lib_path")) if request.param == "emu" else request.getfixturevalue("gpu_hooks_kw")
    e = pkg.ZstdEncoder(level=3, **kw)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model():
    cache = {}
    def get(name, fast, mode):
        if (name, fast, mode) not in cache:
            cache[(name, fast, mode)] = K.model_lists(K.build(name, 8192 if fast else 16384), fast, mode)
        return cache[(name, fast, mode)]
    return get


@pytest.mark.parametrize("name", K.MODEL_NAMES)
@pytest.mark.parametrize("mode", [K.MODE_BASE, K.MODE_FAR], ids=["base", "far"])
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "wide"])
def test_lists_match_model(enc, inputs, model, fast, mode, name):
    x = inputs(name, 8192 if fast else 16384)
    offs, ent = enc.mf_lists(x, fast, mode, K.FRAME_BLOCKS)
    counts, entries = model(name, fast, mode)
    pos_mask = np.uint64((1 << (23 if fast else 24)) - 1)
    assert offs.shape[0] == counts.shape[0] == len(entries)
    for f in range(offs.shape[0]):
        # W1 (+ W2): offsets in (partition, tile) order -> counts per (tile, partition)
        starts = offs[f, :-1, :].T.ravel().astype(np.int64)
        ends = offs[f, -1, :].astype(np.int64)
        total = int(ends[-1])
        got = np.diff(np.concatenate([starts, [total]])).reshape(offs.shape[2], -1).T
        bad = np.argwhere(got != counts[f])
        assert bad.size == 0, "W1, frame %d: tile %d partition %d counts %d positions, the model %d" % (f, bad[0][0], bad[0][1], got[tuple(bad[0])], counts[f][tuple(bad[0])])
        assert np.array_equal(ends[:-1], offs[f, 0, 1:]) and total == entries[f].size, "W2, frame %d: partition ends" % f
        # W3: every entry where the model puts it, nothing behind the last run, positions ascending inside every partition's list
        e = ent[f, :total]
        bad = np.flatnonzero(e != entries[f])
        assert bad.size == 0, "W3, frame %d: entry %d is %#x (position %d), the model has %#x (position %d)" % (
            f, bad[0], int(e[bad[0]]), int(e[bad[0]] & pos_mask), int(entries[f][bad[0]]), int(entries[f][bad[0]] & pos_mask))
        assert np.all(ent[f, total:] == np.uint64(0xFFFFFFFFFFFFFFFF)), "W3, frame %d: an entry written outside the runs" % f
        pos = (e & pos_mask).astype(np.int64)
        lists = np.concatenate([[0], ends])
        for g in range(ends.size):
            assert np.all(np.diff(pos[lists[g]:lists[g + 1]]) > 0), "W3, frame %d: positions of partition %d do not ascend" % (f, g)


def test_the_shipped_library_has_no_lists_entry(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        pytest.skip("shipped library not built")
    assert getattr(pkg.load_library(), "gc_test_mf_lists", None) is None
