"""bench.py --dump-outputs, on the host: what the timed path returned is written exactly, and a result above the budget
is cut down to the same seeded rows every time."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

MODES = ((False, False), (True, True))


def _results(seed, n_fam=500):
    rng = np.random.default_rng(seed)
    out = []
    for _ in MODES:
        sizes = rng.integers(1, 6, n_fam)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        sds = rng.integers(0, 6_000_000_000, (int(offs[-1]), 4), dtype=np.int64).astype(np.uint64)
        out.append((offs, sds))
    return out


def test_dump_is_exact_under_the_budget(tmp_path):
    res = _results(1)
    written = bench.dump_outputs(str(tmp_path), res, MODES)
    assert sorted(written) == sorted(os.listdir(tmp_path))
    for tag, (offs, sds) in zip(("direct", "revcomp"), res):
        o = np.load(tmp_path / f"{tag}_family_offsets.npy")
        d = np.load(tmp_path / f"{tag}_proto_sds.npy")
        assert o.dtype == np.float64 and d.dtype == np.float64 and d.shape == sds.shape
        assert np.array_equal(o.astype(np.uint64), offs) and np.array_equal(d.astype(np.uint64), sds)


def test_dump_above_the_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    res = _results(2, n_fam=4000)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100_000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), res, MODES)
    bench.dump_outputs(str(b), res, MODES)
    total = sum(os.path.getsize(a / f) - 128 for f in os.listdir(a))   # (128: the .npy header)
    assert total <= 100_000
    for f in os.listdir(a):
        assert np.array_equal(np.load(a / f), np.load(b / f)), f
    rows = np.load(a / "revcomp_proto_sds_rows.npy").astype(np.int64)
    assert len(rows) > 0 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(a / "revcomp_proto_sds.npy").astype(np.uint64), res[1][1][rows])
