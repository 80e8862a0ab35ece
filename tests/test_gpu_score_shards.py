"""--compute-score over several shards on the GPU: the union of asgart_compute_scores_shard over N = 1..4 shards, and
asgart_compute_scores_multi over two replicas, are bit-equal to asgart_compute_scores and to the oracle; a whole run on
two ranks (multi.search_duplications through the `python -m asgart_amd.multi` launcher, gloo, one device) writes the
same JSON bytes as the single-GPU driver."""
import os

import numpy as np
import pytest

import asgart_amd
import oracle
from asgart_amd import multi, postprocess, synth
from test_postprocess import _case


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tandem_text():
    """The large-family case of test_postprocess.test_native_chain_large_family: one tandem array."""
    rng = np.random.default_rng(3)
    mono = rng.integers(0, 4, size=171)
    arr = np.tile(mono, 700)
    mut = rng.random(arr.shape) < 0.03
    arr[mut] = (arr[mut] + rng.integers(1, 4, size=int(mut.sum()))) & 3
    g = np.concatenate([rng.integers(0, 4, size=20_000), arr, rng.integers(0, 4, size=20_000)])
    return np.concatenate([np.frombuffer(b"ACGT", dtype=np.uint8)[g], np.frombuffer(b"$", dtype=np.uint8)])


def _with_long_rows(text, sds, seed):
    """The search's survivors plus arms for both kernels' bands (one wave; the 16-wave pipeline from 8192 rows on)."""
    rng = np.random.default_rng(seed)
    n = len(text) - 1
    extra = []
    for ll, rl in [(1, 1), (4095, 100), (8191, 300), (8192, 8192), (20000, 1000), (17000, 21000), (9000, 1)]:
        extra.append((int(rng.integers(0, n - ll - 1)), int(rng.integers(0, n - rl - 1)), ll, rl))
    return np.concatenate([sds, np.array(extra, dtype=np.uint64)])


def _oracle(text, sds, rc, cell_budget=None):
    """Oracle identities, all of them or (cell_budget) the smallest duplications up to that many DP cells in all."""
    # (with a budget the large duplications are compared between entry points only; tests/test_gpu_score_reach.py has
    # arms of up to 66 000 bases, and more pairs than waves and workgroups, against the oracle and a banded reference)
    cells = (sds[:, 2] + 1).astype(np.float64) * (sds[:, 3] + 1)
    pick = np.arange(len(sds))
    if cell_budget is not None:
        order = np.argsort(cells, kind="stable")
        pick = order[:max(1, int((np.cumsum(cells[order]) <= cell_budget).sum()))]
    return pick, np.array([oracle.levenshtein_identity(text, sds[q], rc, rc) for q in pick], dtype=np.float32)


def _check_shards(idx, text, sds, rc, cell_budget=None):
    whole = idx.compute_scores(sds, rc, rc)
    pick, want = _oracle(text, sds, rc, cell_budget)
    assert len(pick) > 0 and np.array_equal(_bits(whole[pick]), _bits(want))
    for n_shards in (1, 2, 3, 4):
        owner = asgart_amd.score_owners(sds, n_shards)
        union = np.full(len(sds), np.nan, dtype=np.float32)
        for r in range(n_shards):
            part = idx.compute_scores_shard(sds, rc, rc, shard=r, n_shards=n_shards)
            mine = owner == r
            assert np.isnan(part[~mine]).all(), (n_shards, r)       # nothing written outside the shard
            assert not np.isnan(part[mine]).any(), (n_shards, r)
            union[mine] = part[mine]
        assert np.array_equal(_bits(union), _bits(whole)), n_shards
    clone = idx.clone(0)
    try:
        both = asgart_amd.compute_scores_multi([idx, clone], sds, rc, rc)
    finally:
        clone.close()
    assert np.array_equal(_bits(both), _bits(whole))
    return whole


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [31, 32, 34])
@pytest.mark.parametrize("rc", [False, True])
def test_shards_equal_one_call_and_oracle(hiplib, seed, rc):
    pr, oidx = _case(seed, short_n_per_mb=60)
    st = asgart_amd.RunSettings.from_cli(min_length=300, reverse=rc, complement=rc)
    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        offs, sds = idx.search_duplications_raw(pr.chunks, st)
        _, kept = idx.post_process(offs, sds)
        assert len(kept) > 3
        sds = _with_long_rows(pr.data, kept, seed)
        _check_shards(idx, pr.data, sds, rc)


@pytest.mark.gpu
@pytest.mark.parametrize("rc", [False, True])
def test_shards_of_the_large_family(hiplib, rc):
    """A tandem array: thousands of duplications in one family before the reduction, arms of 100 kb and more after it.
    (Its -RC pass finds nothing: the direct pass's duplications are scored in both orientations.)"""
    text = _tandem_text()
    st = asgart_amd.RunSettings.from_cli()
    with asgart_amd.Index(text, None) as idx:
        offs, sds = idx.search_duplications_raw([(0, len(text) - 1)], st)
        assert len(sds) > 500
        # the raw duplications (many, similar lengths) and the survivors of the steps behind the search
        _, kept = idx.post_process(offs, sds)
        for arr in (sds, kept):
            _check_shards(idx, text, arr, rc, cell_budget=3e9)


@pytest.mark.gpu
def test_shard_arguments(hiplib):
    text = _tandem_text()
    sds = np.array([[10, 500, 100, 120], [50, 900, 300, 280]], dtype=np.uint64)
    with asgart_amd.Index(text, None) as idx:
        for shard, n in ((2, 2), (-1, 2), (0, 0)):
            with pytest.raises(asgart_amd.AsgartError):
                idx.compute_scores_shard(sds, shard=shard, n_shards=n)
        # the whole list is checked on every shard, also where the bad entry belongs to another one
        bad = np.concatenate([sds, np.array([[len(text) - 5, 0, 10, 3]], dtype=np.uint64)])
        for r in range(3):
            with pytest.raises(asgart_amd.AsgartError) as e:
                idx.compute_scores_shard(bad, shard=r, n_shards=3)
            assert "past the end" in str(e.value)
        with pytest.raises(asgart_amd.AsgartError) as e:
            asgart_amd.compute_scores_multi([idx, idx], bad)
        assert "past the end" in str(e.value)
        assert len(idx.compute_scores_shard(sds[:0], shard=1, n_shards=2)) == 0


def _write_fasta(path, records):
    with open(path, "w") as fh:
        for name, seq in records:
            fh.write(f">{name} synthetic\n")
            s = bytes(seq).decode()
            for o in range(0, len(s), 70):
                fh.write(s[o:o + 70] + "\n")


@pytest.mark.gpu
def test_two_ranks_write_the_single_gpu_json(hiplib, tmp_path):
    """Two gloo ranks on device 0 (at most three processes with the GPU open: this one and the two ranks), started by
    the launcher, each child under the launcher's time limit; the first run that fails ends the test."""
    recs = synth.make_genome([160_000, 110_000, 90_000], seed=23, sd_per_mb=50, sd_len=(1000, 7000), alu_frac=0.05,
                             l1_frac=0.01, sat_per_record=1, sat_copies=(20, 60), short_n_per_mb=20)
    files = [str(tmp_path / "a.fa"), str(tmp_path / "b.fasta")]
    _write_fasta(files[0], recs[:2])
    _write_fasta(files[1], recs[2:])
    for rc in (False, True):
        st = asgart_amd.RunSettings.from_cli(reverse=rc, complement=rc)
        want = postprocess.to_json(postprocess.search_duplications(files, st, 0, compute_score=True))
        assert want.count('"identity": ') > 3 and '"identity": 0.0' not in want
        out = tmp_path / ("rc" if rc else "direct")
        out.mkdir()
        argv = ["--gpus", "2", "--one-device", "--compute-score", "--out-dir", str(out)] + (["-R", "-C"] if rc else []) + files
        assert multi.launch(argv, timeout=600) == 0, rc
        name = postprocess.out_filename(files, st)
        assert sorted(os.listdir(out)) == [name]
        assert (out / name).read_text(encoding="utf-8") == want, rc
