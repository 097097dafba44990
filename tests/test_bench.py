"""bench.py's output dump: dump_outputs on host arrays (CPU), and a small plain run on the device (-m gpu) whose dump of the last timed step is the
stream itself and decodes to the corpus."""
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("gc_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _load(d, tag):
    return [np.load(os.path.join(d, "%s_%s.npy" % (tag, f))) for f in ("stream_size", "stream_sample", "stream_sample_offsets")]


def test_dump_of_a_small_stream_is_the_whole_stream(tmp_path):
    B = _bench()
    s = np.random.default_rng(1).integers(0, 256, 100_000, dtype=np.uint8)
    B.dump_outputs(str(tmp_path), "t", s)
    size, sample, offs = _load(tmp_path, "t")
    assert size.dtype == np.float64 and sample.dtype == np.float32 and offs.dtype == np.float64
    assert size.tolist() == [s.size] and offs.tolist() == [0.0] and sample.shape == (1, s.size)
    assert np.array_equal(sample[0].astype(np.uint8), s)


def test_dump_of_a_large_stream_is_a_fixed_sample_under_the_budget(tmp_path):
    B = _bench()
    s = np.random.default_rng(2).integers(0, 256, 5_000_003, dtype=np.uint8)
    for d in ("a", "b"):
        B.dump_outputs(str(tmp_path / d), "t", s)
    (size, sample, offs), (_, sample2, offs2) = _load(tmp_path / "a", "t"), _load(tmp_path / "b", "t")
    assert size.tolist() == [s.size] and sample.shape == (B.DUMP_WINDOWS, B.DUMP_WINDOW)
    assert np.array_equal(offs, offs2) and np.array_equal(sample, sample2)          # seeded: the same windows every run
    assert offs[0] == 0 and np.all(np.diff(offs) >= B.DUMP_WINDOW) and offs[-1] + B.DUMP_WINDOW <= s.size
    for o, row in zip(offs.astype(np.int64), sample):
        assert np.array_equal(row.astype(np.uint8), s[o:o + B.DUMP_WINDOW])
    assert 2 * sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20    # two legs (--full) within 64 MB


def test_corpus_generator_loads_without_writing_into_the_tree(tmp_path):
    """A tree whose corpus library was never built (or is older than its source), and may be read-only: bench.py builds the library outside
    it and generates the same bytes."""
    B = _bench()
    here = tmp_path / "7-zip-zstd_amd" / "corpus"
    here.mkdir(parents=True)
    for f in ("__init__.py", "corpus_gen.c"):
        shutil.copy2(os.path.join(ROOT, "7-zip-zstd_amd", "corpus", f), here / f)
    os.chmod(here, 0o555)
    try:
        x = B.load_corpus_module(str(tmp_path)).corpus("text-zipf", 100_000)
        assert sorted(f for f in os.listdir(here) if f != "__pycache__") == ["__init__.py", "corpus_gen.c"]
    finally:
        os.chmod(here, 0o755)
    assert np.array_equal(x, B.load_corpus_module(ROOT).corpus("text-zipf", 100_000))


@pytest.mark.gpu
def test_gpu_plain_bench_run_dumps_its_last_step(O, tmp_path):
    n = 8 << 20
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--codec", "zstd", "--bytes", str(n), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert "roofline" not in line and "cpu_baseline" not in line                    # --full only
    size, sample, offs = _load(out, "zstd_l3")
    assert int(size[0]) == line["compressed_bytes"] and sample.shape == (1, line["compressed_bytes"])     # < 4 MiB: the whole stream
    x = O.corpus("text-zipf", n)
    assert np.array_equal(O.port_zstd_decompress(sample[0].astype(np.uint8), n), x)
