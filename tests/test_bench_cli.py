"""bench.py's command line and its --dump-outputs writer, on the CPU: the dump's arrays, its budget and its seeded samples."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _batch(n_docs, max_ids, id_hi, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_ids, n_docs)
    offs = np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)
    ids = rng.integers(0, id_hi, int(offs[-1])).astype(np.uint32)
    return ids, offs


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("doc_index", "token_counts", "id_sums", "ids_index", "ids")}


def test_dump_small_batch_is_whole(tmp_path):
    """A batch that fits the budget is dumped whole: every document, every id (float32: all ids are below 2^24)."""
    ids, offs = _batch(3000, 40, 130072, 1)
    info = _bench().dump_outputs(str(tmp_path), ids, offs)
    a = _load(str(tmp_path))
    assert info["docs_covered"] == 3000 and info["ids_sampled"] == len(ids)
    assert np.array_equal(a["doc_index"], np.arange(3000)) and np.array_equal(a["ids_index"], np.arange(len(ids)))
    assert a["ids"].dtype == np.float32 and np.array_equal(a["ids"], ids)
    assert np.array_equal(a["token_counts"], np.diff(offs.astype(np.int64)))
    o = offs.astype(np.int64)
    assert np.array_equal(a["id_sums"], [int(ids[o[d]:o[d + 1]].sum(dtype=np.int64)) for d in range(3000)])
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())


@pytest.mark.parametrize("n_docs,id_hi", [(1_000_000, 130072), ((1 << 20) + 5000, 1 << 25)])
def test_dump_large_batch_is_a_seeded_sample_within_budget(tmp_path, n_docs, id_hi):
    """More ids than the budget holds -- on the headline shape's 1 M documents, and on more documents than 2^20 with ids of 2^24 and
    above (written as float64): seeded sorted samples, the same from run to run, 64 MB (64 x 10^6 bytes) of files at most, .npy headers
    included."""
    ids, offs = _batch(n_docs, 24, id_hi, 2)
    bench = _bench()
    info = bench.dump_outputs(str(tmp_path / "a"), ids, offs)
    bench.dump_outputs(str(tmp_path / "b"), ids, offs)
    on_disk = sum(os.path.getsize(str(f)) for f in (tmp_path / "a").iterdir())
    assert on_disk == info["bytes"] <= 64_000_000 and len(list((tmp_path / "a").iterdir())) == 5
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    docs = a["doc_index"].astype(np.int64)
    assert len(docs) == min(n_docs, 1 << 20) and np.all(np.diff(docs) > 0) and docs[-1] < len(offs) - 1
    pos = a["ids_index"].astype(np.int64)
    assert 0 < len(pos) < len(ids) and np.all(np.diff(pos) > 0) and pos[-1] < len(ids)
    assert a["ids"].dtype == (np.float64 if id_hi > 1 << 24 else np.float32) and np.array_equal(a["ids"], ids[pos])
    o = offs.astype(np.int64)
    for j in (0, 1, 777, len(docs) - 1):
        d = docs[j]
        assert a["token_counts"][j] == o[d + 1] - o[d] and a["id_sums"][j] == ids[o[d]:o[d + 1]].sum(dtype=np.int64)


def test_steps_below_one_is_refused():
    """--steps sets the number of timed steps: a count below one is an error, refused before anything is set up."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
