"""The run directory (csrc/run_dir.hpp): the suffix-array interval of every k-mer with at least T occurrences, one 64-byte
bucket per lookup, consulted by kmer_range before the prefix table.  It may only shorten a lookup: the parity surface
(asgart_searcher_search) and whole calls give the oracle's answers with the directory, without it (ASGART_RUN_DIR=0, fresh
child processes: the variable is read when an index is created), with a table of one or two buckets that nearly every run
finds full, and when the table's allocation fails; a clone has a directory of its own.

One text of under 64 kb, built here with a fixed seed: random sequence; 24-bp units tiled 2, 3, 32, 33, 256, 257 and 520
times (the k-mer at a unit's start occurs once per copy, the k-mers across a unit boundary once less: runs of 1, 2, 3 --
T - 1, T and T + 1 at the default T = 2 --, of 32 and 33 around kSmallInterval, of 256 and 257 around kRankMin, and of 520,
above max_cardinality = 500); a run of N; one unit once more as its reverse complement; a 40-bp unit three times, the last
copy ending the text (its k-mers share their first 8 bases with the suffixes shorter than k: the text-tail corner).
test_the_text_holds_the_runs (no GPU) asserts, over the oracle's suffix array, that these run lengths occur."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
K = 20
T = 2                      # kRunDirT: the default ASGART_RUN_DIR_T
CARD = 500                 # max_cardinality of the calls
U = 24                     # bases of a tiled unit (>= every probe size tried)
TILED = (2, 3, 32, 33, 256, 257, CARD + 20)
KS = (8, 20, 21, 22)       # 21: the widest single key word; 22: two words, no directory
DIRECT, RC = (False, False), (True, True)
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = {65: 84, 84: 65, 67: 71, 71: 67, 78: 78}
CHILD_LIMIT_S = 120


def revcomp(a):
    return np.array([COMP[int(c)] for c in a[::-1]], dtype=np.uint8)


def make_text():
    rng = np.random.default_rng(20240611)

    def rand(n):
        return BASES[rng.integers(0, 4, size=n)]

    units = {c: rand(U) for c in TILED}
    tail_unit = rand(40)
    parts = [rand(1500)]
    for c in TILED:
        parts += [np.tile(units[c], c), rand(300)]
    parts += [np.full(40, ord("N"), dtype=np.uint8), rand(400), revcomp(units[33]), rand(400),
              tail_unit, rand(200), tail_unit, rand(700), tail_unit, np.frombuffer(b"$", dtype=np.uint8)]
    text = np.concatenate(parts)
    assert len(text) < 64_000
    return text


def run_lengths(text, sa, k):
    """Lengths of the runs of equal k-mers in suffix-array order (suffixes shorter than k left out), and per text position
    the number of occurrences of the k-mer that starts there."""
    codes = np.searchsorted(np.frombuffer(b"$ACGNT", dtype=np.uint8), text).astype(np.uint64)
    n = len(text)
    key = np.zeros(n - k + 1, dtype=np.uint64)
    for j in range(k):
        key = key * np.uint64(6) + codes[j:n - k + 1 + j]
    in_order = key[sa[sa <= n - k]]
    cut = np.flatnonzero(np.diff(in_order) != 0)
    runs = np.diff(np.concatenate([[-1], cut, [len(in_order) - 1]]))
    _, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    return runs, counts[inv]


def probes_of(text, mode, k):
    """-> (patterns as an (n, k) byte array, their needle offsets): every probe of the one-chunk list in orientation `mode`."""
    L = len(text) - 1
    needle = oracle.prepare_needle(text, (0, L), oracle.make_settings(k=k, reverse=mode[0], complement=mode[1]))
    step = k // 2
    offs = np.arange(step, step * (-(-(L - k - step) // step)) + 1, step)
    return np.stack([needle[i:i + k] for i in offs]), offs


def tail_corner_8mers(text, k):
    """The 8-mers that send a probe down the text-tail path: those of the suffixes shorter than k (the '$' is in none)."""
    n = len(text)
    return {bytes(text[x:x + 8]) for x in range(n - k + 1, n - 8)}


class Case:
    def __init__(self):
        self.text = make_text()
        self.oidx = oracle.Index.build(self.text)
        self.chunks = [(0, len(self.text) - 1)]
        self._ranges, self._fams = {}, {}

    def oracle_ranges(self, k, mode):
        """Per probe the oracle's (lo, hi); (0, 0) where it finds nothing."""
        if (k, mode) not in self._ranges:
            pats, _ = probes_of(self.text, mode, k)
            seen, out = {}, np.zeros((len(pats), 2), dtype=np.uint64)
            for j, p in enumerate(pats):
                b = bytes(p)
                if b not in seen:
                    hits, (lo, hi) = self.oidx.search(b)
                    assert len(hits) == 0 or hi - lo == len(hits)
                    seen[b] = (lo, hi) if len(hits) else (0, 0)
                out[j] = seen[b]
            out.setflags(write=False)
            self._ranges[(k, mode)] = out
        return self._ranges[(k, mode)]

    def oracle_families(self, mode):
        if mode not in self._fams:
            st = oracle.make_settings(k=K, reverse=mode[0], complement=mode[1], max_cardinality=CARD)
            self._fams[mode] = self.oidx.run_raw(self.chunks, st, threads=2)
        return self._fams[mode]


@pytest.fixture(scope="module")
def case():
    return Case()


def settings(mode):
    return asgart_amd.RunSettings.from_cli(k=K, reverse=mode[0], complement=mode[1], max_cardinality=CARD)


def gpu_ranges(idx, text, k, mode):
    pats, _ = probes_of(text, mode, k)
    got = asgart_amd.Searcher(idx).search_ranges([bytes(p) for p in pats])
    return np.array(got, dtype=np.uint64).reshape(-1, 2)


def assert_ranges(got, want, what):
    assert got.shape == want.shape, what
    found = want[:, 1] > want[:, 0]
    assert np.array_equal(got[found], want[found]), what
    assert np.array_equal(got[~found, 0], got[~found, 1]), what


def assert_whole_calls(idx, case, what, sharded=True):
    """A direct run, an -RC run, the two as one job and the direct run cut into 3 shards, against the oracle."""
    want = [case.oracle_families(m) for m in (DIRECT, RC)]
    assert sum(len(w[1]) for w in want) > 0
    for m, (eoffs, esds) in zip((DIRECT, RC), want):
        offs, sds = idx.search_duplications_raw(case.chunks, settings(m))
        assert np.array_equal(offs, eoffs) and np.array_equal(sds, esds), (what, m)
    for (offs, sds), (eoffs, esds) in zip(idx.search_duplications_passes(case.chunks, [settings(DIRECT), settings(RC)]), want):
        assert np.array_equal(offs, eoffs) and np.array_equal(sds, esds), (what, "passes")
    if sharded:
        parts = [idx.search_duplications_raw(case.chunks, settings(DIRECT), shard=r, n_shards=3, with_keys=True) for r in range(3)]
        offs, sds = asgart_amd.merge_shards(parts)
        assert np.array_equal(offs, want[0][0]) and np.array_equal(sds, want[0][1]), (what, "3 shards")


# ---- no GPU ---------------------------------------------------------------------------------------------------------------
def test_the_text_holds_the_runs(case):
    text, sa = case.text, case.oidx.sa
    runs, occ = run_lengths(text, sa, K)
    have = set(runs.tolist())
    assert {1, T - 1, T, T + 1, 32, 33, 256, 257} <= have
    assert max(have) == CARD + 20 > CARD
    # probes (stride k / 2) meet them too: the directory is asked for runs on both sides of every seam
    _, offs = probes_of(text, DIRECT, K)
    met = set(occ[offs].tolist())
    assert {1, 2, 3, 32, 33, 256, 257, CARD + 20} <= met
    # an N run, and k-mers with an N inside that are looked up all the same
    pats, _ = probes_of(text, DIRECT, K)
    assert any(p[0] == ord("N") for p in pats) and any(p[0] != ord("N") and ord("N") in p for p in pats)
    # the text ends inside a repeat: probes of the earlier copies take the text-tail path
    corner = tail_corner_8mers(text, K)
    assert sum(bytes(p[:8]) in corner for p in pats) >= 2
    # the reverse-complemented unit: the -RC pass finds the array of 33
    want = case.oracle_ranges(K, RC)
    assert int((want[:, 1] - want[:, 0]).max()) >= 33


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _child(switch, tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASGART_RUN_DIR")}
    env["ASGART_RUN_DIR"] = str(switch)
    out = os.path.join(str(tmp_path), f"ranges_{switch}.npz")
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(HERE, "run_dir_child.py"), out],
                       env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S + 60)
    tail = f"exit {p.returncode}\n--- stdout\n{p.stdout[-3000:]}\n--- stderr\n{p.stderr[-3000:]}"
    assert p.returncode == 0, tail
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, tail
    return np.load(out), json.loads(lines[0])


@pytest.mark.gpu
def test_searcher_parity_with_and_without_the_directory(case, tmp_path):
    """asgart_searcher_search for every probe of the text, direct and -RC, at k = 8, 20, 21 and 22: the oracle's
    intervals, and the same with ASGART_RUN_DIR=0 and =1."""
    off, info_off = _child(0, tmp_path)
    on, info_on = _child(1, tmp_path)
    for k in KS:
        for name, mode in (("direct", DIRECT), ("rc", RC)):
            want = case.oracle_ranges(k, mode)
            key = f"k{k}_{name}"
            assert_ranges(on[key], want, (key, "on"))
            assert_ranges(off[key], want, (key, "off"))
            assert np.array_equal(on[key], off[key]), key
        assert info_off[str(k)]["bytes"] == 0 and info_off[str(k)]["switch"] == 0
        if k <= 21:
            assert info_on[str(k)]["bytes"] == 64 * info_on[str(k)]["buckets"] > 0 and info_on[str(k)]["T"] == T, k
            assert info_on[str(k)]["inserted"] > 0
        else:   # two key words: no directory
            assert info_on[str(k)]["bytes"] == 0 and info_on[str(k)]["buckets"] == 0, k


@pytest.mark.gpu
def test_whole_calls(case):
    with asgart_amd.Index(case.text, case.oidx.sa) as idx:
        assert_whole_calls(idx, case, "default")
        assert idx.run_dir_info()["bytes"] > 0


@pytest.mark.gpu
def test_whole_calls_with_64_bit_slots(case, monkeypatch):
    monkeypatch.setenv("ASGART_FORCE_WIDE", "1")
    with asgart_amd.Index(case.text, case.oidx.sa) as idx:
        assert_whole_calls(idx, case, "wide", sharded=False)
        assert idx.run_dir_info()["bytes"] > 0
        assert_ranges(gpu_ranges(idx, case.text, K, DIRECT), case.oracle_ranges(K, DIRECT), "wide")


@pytest.mark.gpu
@pytest.mark.parametrize("buckets", (1, 2))
def test_a_starved_directory(case, buckets, monkeypatch):
    """One or two buckets: nearly every run finds its bucket full and is looked up through the prefix table."""
    monkeypatch.setenv("ASGART_RUN_DIR_BUCKETS", str(buckets))
    with asgart_amd.Index(case.text, case.oidx.sa) as idx:
        idx.prepare(K)
        info = idx.run_dir_info()
        assert info["buckets"] == buckets and info["bytes"] == 64 * buckets
        assert info["inserted"] == 4 * buckets and info["bucket_full"] > 100
        assert_whole_calls(idx, case, ("starved", buckets))
        for mode in (DIRECT, RC):
            assert_ranges(gpu_ranges(idx, case.text, K, mode), case.oracle_ranges(K, mode), ("starved", buckets, mode))


@pytest.mark.gpu
def test_the_index_goes_without_when_the_allocation_fails(case):
    """test_fail_alloc aimed at the table's allocation: prepare succeeds, the index has no directory, same results."""
    found = False
    for nth in range(8):   # (the allocations of prepare in front of the table's fail the prepare itself)
        with asgart_amd.Index(case.text, case.oidx.sa) as idx:
            idx.set_option("test_fail_alloc", nth)
            try:
                idx.prepare(K)
            except asgart_amd.AsgartError:
                continue
            finally:
                idx.set_option("test_fail_alloc", -1)
            if idx.run_dir_info()["bytes"] == 0:
                found = True
                assert idx.run_dir_info()["switch"] == 1
                assert_whole_calls(idx, case, "no memory", sharded=False)
                assert_ranges(gpu_ranges(idx, case.text, K, DIRECT), case.oracle_ranges(K, DIRECT), "no memory")
                break
    assert found


@pytest.mark.gpu
def test_a_clone_has_a_directory_of_its_own(case):
    with asgart_amd.Index(case.text, case.oidx.sa) as idx:
        idx.prepare(K)
        with idx.clone() as twin:
            for mode in (DIRECT, RC):
                a, b = gpu_ranges(idx, case.text, K, mode), gpu_ranges(twin, case.text, K, mode)
                assert np.array_equal(a, b), mode
                assert_ranges(b, case.oracle_ranges(K, mode), ("clone", mode))
            src, dst = idx.run_dir_info(), twin.run_dir_info()
            assert dst["bytes"] == src["bytes"] > 0 and dst["T"] == src["T"]
            assert dst["inserted"] + dst["bucket_full"] == src["inserted"] + src["bucket_full"]


@pytest.mark.gpu
def test_hits_and_misses(case, monkeypatch):
    """A fresh index, one direct call: its position bits were blank, so the accounting pass looks every probe up (those
    that start with N are never looked up).  No run found its bucket full, so every probe whose k-mer occurs at least T
    times, the text-tail corner's apart, is answered by the directory, and no other.  (At the default size -- a load of
    one half, 88 buckets for this text's 176 runs -- two runs find their bucket full, as buckets of four at that load
    will: the table is enlarged here so that none does.)"""
    monkeypatch.setenv("ASGART_RUN_DIR_BUCKETS", "4096")
    text = case.text
    pats, offs = probes_of(text, DIRECT, K)
    _, occ = run_lengths(text, case.oidx.sa, K)
    corner = tail_corner_8mers(text, K)
    looked_up = np.array([p[0] != ord("N") for p in pats])
    in_corner = np.array([bytes(p[:8]) in corner for p in pats])
    want_hits = int(np.sum(looked_up & ~in_corner & (occ[offs] >= T)))
    want_misses = int(np.sum(looked_up & ~in_corner & (occ[offs] < T)))
    assert want_hits > 0 and want_misses > 0 and int(np.sum(in_corner)) > 0
    with asgart_amd.Index(text, case.oidx.sa) as idx:
        idx.search_duplications_raw(case.chunks, settings(DIRECT))
        st = idx.stats(1)
        info = idx.run_dir_info()
        acct = idx.lookup_account()
    assert info["bucket_full"] == 0 and info["T"] == T and info["buckets"] == 4096
    runs, _ = run_lengths(text, case.oidx.sa, K)
    assert info["inserted"] == int(np.sum(runs >= T))
    assert (info["hits"], info["misses"]) == (want_hits, want_misses)
    assert (acct["dir_hits"], acct["dir_misses"]) == (want_hits, want_misses)
    # a hit reads nothing from the prefix table; a miss reads it once (unless an N among its first bases keeps it out)
    assert 0 < acct["ptab_loads"] <= want_misses and acct["keys_loads"] > 0
    assert st.search_bytes > 0
