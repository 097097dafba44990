"""The wave scans of csrc/gc_device.h that go through DPP moves instead of the LDS crossbar (gc_wave_incl_sum_dpp, gc_wave_incl_max_dpp, gc_wave_incl_max64_dpp; the
sequence stage of the zstd encoder is their user), against numpy, through the test entry gc_test_wave_scans: one wave per 64 values.  Under the emulator the helpers are
the shuffle loops; on the device they are six DPP moves each, and a row shift, a row broadcast or the half-wave broadcast that reads the wrong lane shows here: the
inputs put a single 1 in front of and behind every row edge (lanes 15 | 16, 47 | 48) and the half-wave edge (31 | 32)."""
import numpy as np
import pytest

EDGE_LANES = (0, 15, 16, 31, 32, 63)


def _cases():
    """name -> (values, keys): whole waves of 64, several per case"""
    rng = np.random.default_rng(950)
    zeros, ones = np.zeros(64, np.uint32), np.ones(64, np.uint32)
    cases = {"zeros": (zeros, zeros.astype(np.uint64)), "ones": (ones, ones.astype(np.uint64))}
    for lane in EDGE_LANES:
        v = zeros.copy()
        v[lane] = 1
        cases["one_in_lane_%d" % lane] = (v, v.astype(np.uint64) << np.uint64(32 * (lane & 1)))       # (the key's 1 in the low half or the high half)
    big = rng.integers(0, 1 << 32, 64 * 8, dtype=np.uint64)
    cases["random_wrapping"] = (big.astype(np.uint32), rng.integers(0, 1 << 63, 64 * 8, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 64 * 8, dtype=np.uint64))
    # keys whose low halves order against their high halves: the larger key has the smaller low half, and the other way round
    hi, lo = rng.integers(0, 4, 64 * 4, dtype=np.uint64), rng.integers(0, 1 << 32, 64 * 4, dtype=np.uint64)
    cases["key_halves_disagree"] = (lo.astype(np.uint32), (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - lo) // (hi + np.uint64(1)))
    cases["key_high_halves_equal"] = (lo.astype(np.uint32), (np.uint64(7) << np.uint64(32)) | lo)
    same = np.full(64, (123 << 32) | 456, np.uint64)
    cases["keys_equal"] = (np.full(64, 5, np.uint32), same)
    grow = (np.arange(2, 66, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 24, 64, dtype=np.uint64)     # the sequence stage's keys: (index + 2, offset), 0 between
    grow[rng.integers(0, 2, 64) == 0] = 0
    cases["run_keys"] = (rng.integers(0, 5, 64, dtype=np.uint64).astype(np.uint32), grow)
    return cases


CASES = _cases()


def _expected(v, keys):
    v2, k2 = v.reshape(-1, 64), keys.reshape(-1, 64)
    return (np.cumsum(v2.astype(np.uint64), axis=1).astype(np.uint32).ravel(), np.maximum.accumulate(v2, axis=1).ravel(), np.maximum.accumulate(k2, axis=1).ravel())


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def enc(request, pkg):
    kw = dict(lib_path=request.getfixturevalue("emu_lib_path")) if request.param == "emu" else request.getfixturevalue("gpu_hooks_kw")
    e = pkg.ZstdEncoder(level=3, **kw)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_wave_scans(enc, name):
    v, keys = CASES[name]
    s, mx, mx64 = enc.wave_scans(v, keys)
    es, emx, emx64 = _expected(v, keys)
    assert np.array_equal(s, es), "%s: inclusive sum, first difference in lane %d" % (name, int(np.flatnonzero(s != es)[0]) % 64)
    assert np.array_equal(mx, emx), "%s: inclusive max, first difference in lane %d" % (name, int(np.flatnonzero(mx != emx)[0]) % 64)
    assert np.array_equal(mx64, emx64), "%s: inclusive 64-bit max, first difference in lane %d" % (name, int(np.flatnonzero(mx64 != emx64)[0]) % 64)


def test_all_cases_in_one_call(enc):
    """every case's waves side by side in one launch (many workgroups), and a length that is no multiple of 64"""
    v = np.concatenate([CASES[k][0] for k in sorted(CASES)] + [np.arange(1, 38, dtype=np.uint32)])
    keys = np.concatenate([CASES[k][1] for k in sorted(CASES)] + [np.arange(37, 0, -1, dtype=np.uint64) << np.uint64(31)])
    s, mx, mx64 = enc.wave_scans(v, keys)
    pad = (-v.size) % 64
    es, emx, emx64 = _expected(np.concatenate([v, np.zeros(pad, np.uint32)]), np.concatenate([keys, np.zeros(pad, np.uint64)]))
    assert np.array_equal(s, es[:v.size]) and np.array_equal(mx, emx[:v.size]) and np.array_equal(mx64, emx64[:v.size])


def test_the_shipped_library_has_no_scan_entry(pkg):
    import os
    if os.path.exists(pkg.LIB_PATH):
        assert getattr(pkg.load_library(), "gc_test_wave_scans", None) is None
