"""Several orientations in one run, on the GPU: asgart_compute_scores_flags* against the calls with one pair of flags
(bit for bit) and the oracle, their shards, and the run over a list of orientations (postprocess.search_orientations, the
`python -m asgart_amd.multi --orientations` launcher) against one run per orientation and the merge of their files."""
import os

import numpy as np
import pytest

import asgart_amd
import oracle
from asgart_amd import extract, multi, postprocess, synth
from test_gpu_score_shards import _bits, _tandem_text, _with_long_rows, _write_fasta
from test_postprocess import _case

ORIENTATIONS = {"direct": (False, False), "R": (True, False), "C": (False, True), "RC": (True, True)}


def _mixed_flags(sds, seed):
    """Flag bytes drawn with a fixed seed; every value among the long rows (the 16-wave kernel) and among the rest."""
    rng = np.random.default_rng(seed)
    flags = rng.integers(0, 4, size=len(sds)).astype(np.uint8)
    long_rows = np.flatnonzero(sds[:, 2] + 1 >= 8192)
    short_rows = np.flatnonzero(sds[:, 2] + 1 < 8192)
    for rows in (long_rows, short_rows):
        assert len(rows) >= 4
        flags[rows[:4]] = [0, 1, 2, 3]
    return flags


def _check_flags(idx, text, sds, seed, cell_budget):
    uniform = [idx.compute_scores(sds, bool(f & 1), bool(f >> 1)) for f in range(4)]
    for f in range(4):
        got = idx.compute_scores_flags(sds, np.full(len(sds), f, dtype=np.uint8))
        assert np.array_equal(_bits(got), _bits(uniform[f])), f
    assert np.array_equal(_bits(idx.compute_scores_flags(sds, None)), _bits(uniform[0]))
    flags = _mixed_flags(sds, seed)
    want = np.array([uniform[f][q] for q, f in enumerate(flags.tolist())], dtype=np.float32)
    whole = idx.compute_scores_flags(sds, flags)
    assert np.array_equal(_bits(whole), _bits(want))
    # the small duplications against the oracle, each with its own flags (the large ones are compared between entry
    # points only; tests/test_gpu_score_reach.py scores long arms with mixed flags against the oracle and a banded reference)
    cells = (sds[:, 2] + 1).astype(np.float64) * (sds[:, 3] + 1)
    order = np.argsort(cells, kind="stable")
    pick = order[:max(1, int((np.cumsum(cells[order]) <= cell_budget).sum()))]
    ref =np.array([oracle.levenshtein_identity(text, sds[q], bool(flags[q] & 1), bool(flags[q] >> 1)) for q in pick],
                   dtype=np.float32)
    assert len(pick) > 3 and np.array_equal(_bits(whole[pick]), _bits(ref))
    # shards: nothing outside the owner set, the union is the one call
    for n_shards in (1, 2, 3, 4):
        owner = asgart_amd.score_owners(sds, n_shards)
        union = np.full(len(sds), np.nan, dtype=np.float32)
        for r in range(n_shards):
            part = idx.compute_scores_flags_shard(sds, flags, shard=r, n_shards=n_shards)
            mine = owner == r
            assert np.isnan(part[~mine]).all() and not np.isnan(part[mine]).any(), (n_shards, r)
            union[mine] = part[mine]
        assert np.array_equal(_bits(union), _bits(whole)), n_shards
    clone = idx.clone(0)
    try:
        both = asgart_amd.compute_scores_flags_multi([idx, clone], sds, flags)
    finally:
        clone.close()
    assert np.array_equal(_bits(both), _bits(whole))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [31, 34])
def test_flags_equal_uniform_calls_shards_and_oracle(hiplib, seed):
    pr, oidx = _case(seed, short_n_per_mb=60)
    st = asgart_amd.RunSettings.from_cli(min_length=300)
    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        offs, sds = idx.search_duplications_raw(pr.chunks, st)
        _, kept = idx.post_process(offs, sds)
        assert len(kept) > 3
        _check_flags(idx, pr.data, _with_long_rows(pr.data, kept, seed), seed, cell_budget=3e9)


@pytest.mark.gpu
def test_flags_of_the_large_family(hiplib):
    text = _tandem_text()
    with asgart_amd.Index(text, None) as idx:
        offs, sds = idx.search_duplications_raw([(0, len(text) - 1)], asgart_amd.RunSettings.from_cli())
        _, kept = idx.post_process(offs, sds)
        # some of the raw duplications (short arms) and the survivors of the steps behind the search (100 kb and more)
        _check_flags(idx, text, _with_long_rows(text, np.concatenate([sds[:200], kept]), 3), 3, cell_budget=3e9)


@pytest.mark.gpu
def test_a_flag_byte_of_4_is_refused_on_every_shard(hiplib):
    text = _tandem_text()
    sds = np.array([[10, 500, 100, 120], [50, 900, 300, 280], [70, 1900, 30, 28]], dtype=np.uint64)
    bad = np.array([0, 3, 4], dtype=np.uint8)
    with asgart_amd.Index(text, None) as idx:
        with pytest.raises(asgart_amd.AsgartError) as e:
            idx.compute_scores_flags(sds, bad)
        assert e.value.code == -1 and "flag byte 4" in str(e.value)
        for r in range(3):
            with pytest.raises(asgart_amd.AsgartError) as e:
                idx.compute_scores_flags_shard(sds, bad, shard=r, n_shards=3)
            assert e.value.code == -1 and "flag byte 4" in str(e.value)
        with pytest.raises(asgart_amd.AsgartError) as e:
            asgart_amd.compute_scores_flags_multi([idx, idx], sds, bad)
        assert "flag byte 4" in str(e.value)
        assert len(idx.compute_scores_flags_shard(sds[:0], bad[:0], shard=1, n_shards=2)) == 0


def _files(tmp_path):
    recs = synth.make_genome([160_000, 110_000, 90_000], seed=23, sd_per_mb=50, sd_len=(1000, 7000), alu_frac=0.05,
                             l1_frac=0.01, sat_per_record=1, sat_copies=(20, 60), short_n_per_mb=20)
    files = [str(tmp_path / "a.fa"), str(tmp_path / "b.fasta")]
    _write_fasta(files[0], recs[:2])
    _write_fasta(files[1], recs[2:])
    return files


def _single_runs(files, tmp_path):
    """One run per orientation, the way to these files without the feature -> {token: (text, path of its file)}."""
    out = {}
    for tok, (r, c) in ORIENTATIONS.items():
        st = asgart_amd.RunSettings.from_cli(reverse=r, complement=c)
        text = postprocess.to_json(postprocess.search_duplications(files, st, 0, compute_score=True))
        path = tmp_path / ("single_" + postprocess.out_filename(files, st))
        path.write_text(text, encoding="utf-8")
        out[tok] = (text, str(path))
    assert out["direct"][0].count('"identity": ') > 3 and '"identity": 0.0' not in out["direct"][0]
    return out


@pytest.mark.gpu
def test_one_run_over_orientations_gives_every_single_run_and_their_merge(hiplib, tmp_path):
    """Also the launcher on two gloo ranks on device 0: at most three processes hold the GPU at once (this one and the
    two ranks), each child under the launcher's time limit."""
    files = _files(tmp_path)
    single = _single_runs(files, tmp_path)
    base = asgart_amd.RunSettings.from_cli(reverse=True)          # its own two flags are ignored
    for toks in (["direct", "RC"], ["RC", "direct"], ["direct", "R", "C", "RC"]):
        per, merged = postprocess.search_orientations(files, [ORIENTATIONS[t] for t in toks], base, 0, compute_score=True)
        assert len(per) == len(toks)
        for tok, (text, name) in zip(toks, per):
            r, c = ORIENTATIONS[tok]
            assert name == postprocess.out_filename(files, asgart_amd.RunSettings.from_cli(reverse=r, complement=c)), tok
            assert text == single[tok][0], (toks, tok)
        assert merged == postprocess.merge_results([single[t][1] for t in toks]), toks
    out = tmp_path / "launched"
    out.mkdir()
    argv = ["--gpus", "2", "--one-device", "--orientations", "direct,RC", "--compute-score", "--merged", "m.json",
            "--out-dir", str(out)] + files
    assert multi.launch(argv, timeout=600) == 0
    names = [postprocess.out_filename(files, asgart_amd.RunSettings.from_cli(reverse=r, complement=r)) for r in (False, True)]
    assert sorted(os.listdir(out)) == sorted(names + ["m.json"])
    assert (out / names[0]).read_text(encoding="utf-8") == single["direct"][0]
    assert (out / names[1]).read_text(encoding="utf-8") == single["RC"][0]
    assert (out / "m.json").read_text(encoding="utf-8") == postprocess.merge_results(
        [single["direct"][1], single["RC"][1]])


@pytest.mark.gpu
def test_it_really_is_one_run(hiplib, tmp_path, monkeypatch):
    files = _files(tmp_path)
    calls = {"index": 0, "passes": [], "score": 0}
    init, passes, score = (asgart_amd.Index.__init__, asgart_amd.Index.search_duplications_passes,
                           asgart_amd.Index.compute_scores_flags_shard)

    def count_init(self, *a, **k):
        calls["index"] += 1
        return init(self, *a, **k)

    def count_passes(self, chunks, settings, *a, **k):
        calls["passes"].append(len(settings))
        return passes(self, chunks, settings, *a, **k)

    def count_score(self, *a, **k):
        calls["score"] += 1
        return score(self, *a, **k)

    monkeypatch.setattr(asgart_amd.Index, "__init__", count_init)
    monkeypatch.setattr(asgart_amd.Index, "search_duplications_passes", count_passes)
    monkeypatch.setattr(asgart_amd.Index, "compute_scores_flags_shard", count_score)
    per, _ = postprocess.search_orientations(files, [(False, False), (True, True)], asgart_amd.RunSettings.from_cli(), 0,
                                             compute_score=True)
    assert len(per) == 2 and calls == {"index": 1, "passes": [2], "score": 1}


@pytest.mark.gpu
def test_sequences_of_a_run_over_orientations(hiplib, tmp_path, monkeypatch):
    import torch.distributed as dist

    files = _files(tmp_path)
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
        monkeypatch.setenv("MASTER_PORT", str(sk.getsockname()[1]))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        base = asgart_amd.RunSettings.from_cli()
        per, merged = multi.search_orientations(files, [(False, False), (True, True)], base, dist, 0,
                                                with_sequences=True)
        for (text, name), rc in zip(per, (False, True)):
            st = asgart_amd.RunSettings.from_cli(reverse=rc, complement=rc)
            want, want_name = multi.search_duplications(files, st, dist, 0, with_sequences=True)
            assert name == want_name and text == want, rc
            flat = [sd for fam in extract.parse_result(text)["families"] for sd in fam]
            assert flat and all(sd["left_seq"] and sd["right_seq"] for sd in flat)
    finally:
        dist.destroy_process_group()
    both = [sd for fam in extract.parse_result(merged)["families"] for sd in fam]
    singles = [sd for text, _ in per for fam in extract.parse_result(text)["families"] for sd in fam]
    assert [(sd["left_seq"], sd["right_seq"], sd["reversed"]) for sd in both] == \
        [(sd["left_seq"], sd["right_seq"], sd["reversed"]) for sd in singles]


@pytest.mark.gpu
def test_a_list_of_one_orientation_is_the_single_run(hiplib, tmp_path):
    """The seam between the two entry points of the one driver: search_orientations with a single orientation returns what
    search_duplications returns for it -- result text, name and PAF text -- and its merge of one file is that file.  In
    process, with scores and PAF rows, with the default writers and with the host's (the genome of
    test_gpu_align.test_multi_writes_a_paf_file_per_orientation, which has duplications of both orientations)."""
    recs = synth.make_genome([90_000, 60_000], seed=41, sd_per_mb=60, sd_len=(1000, 5000), alu_frac=0.03, l1_frac=0.0,
                             sat_per_record=0, short_n_per_mb=10)
    files = [str(tmp_path / "g.fa")]
    _write_fasta(files[0], recs)
    base = asgart_amd.RunSettings.from_cli(complement=True)          # its own two flags are ignored
    for tok in ("direct", "RC"):
        r, c = ORIENTATIONS[tok]
        st = asgart_amd.RunSettings.from_cli(reverse=r, complement=c)
        for writer in (None, "host"):
            per, merged = multi.search_orientations(files, [(r, c)], base, None, 0, compute_score=True, writer=writer,
                                                    paf=True)
            want = multi.search_duplications(files, st, None, 0, compute_score=True, writer=writer, paf=True)
            assert len(want) == 3 and per == [want], (tok, writer)
            assert want[1] == postprocess.out_filename(files, st) and '"identity": ' in want[0]
            assert len(want[2].splitlines()) >= 1, tok
            path = tmp_path / f"{tok}_{writer}.json"
            path.write_text(per[0][0], encoding="utf-8")
            assert merged == postprocess.merge_results([str(path)]) == per[0][0], (tok, writer)
