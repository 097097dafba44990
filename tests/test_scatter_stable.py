"""The finder's scatter pass (W3, csrc/gc_lz_window.hip mf_scatter_body) is a STABLE counting sort: how many waves share a tile, and how
a position's partition travels from the histogram pass to the ranking pass, are scheduling choices that must not move one compressed byte.

Every case (tests/scatter_cases.py) compresses one input and compares the SHA-256 of the stream with
tests/golden/scatter_stable_sha256.json, which tools/gen_scatter_golden.py recorded at the commit named in the fixture (`_parent_commit`:
the last one with one thread per partition in W3).  The CPU emulator and the device (-m gpu) run the same cases against the same fixture
entries: emulator bytes == device bytes.  The frame-sized inputs take the emulator minutes each at zstd 19, Fast-LZMA2 5 and brotli 6."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "scatter_stable_sha256.json")

_spec = importlib.util.spec_from_file_location("scatter_cases", os.path.join(HERE, "scatter_cases.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

# the longest cases first: spread over worker processes, the frame-sized ones then start together instead of trailing the run
CASES = sorted(S.cases(), key=lambda c: -c[3])


@pytest.fixture(scope="module")
def golden():
    d = json.load(open(GOLDEN))
    assert len(d["_parent_commit"]) == 40
    return d["sha256"]


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(S.case_id(c) for c in S.cases())


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_emulator_stream_unchanged(O, pkg, emu_lib_path, golden, case):
    assert S.stream_sha256(pkg, O.corpus, case, lib_path=emu_lib_path) == golden[S.case_id(case)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_gpu_stream_unchanged(O, pkg, gpu_enc, golden, case):
    assert S.stream_sha256(pkg, O.corpus, case, device=0) == golden[S.case_id(case)]
