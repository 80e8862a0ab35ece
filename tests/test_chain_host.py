"""chain.chain_host, the per-object statement of the chaining rule (include/asgart_hip.h), without a GPU: against a brute
force that enumerates every increasing path of links, the four properties of the rule on random cases, the window, the
constructed branch cases (random data almost never cuts a link), the TSV and the chained result on a worked example, and
the refusals.  Every test asserts that the case it is about occurred."""
import itertools

import numpy as np
import pytest

from asgart_amd import chain
from asgart_amd import slice as sl

M64 = 2 ** 64 - 1
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}


def anchors(rows, flag=0, names=(0, 0)):
    """rows of (pl, pr, ll, rl) -> the arguments of chain_host for one group."""
    rows = np.asarray(rows, dtype=object).reshape(-1, 4)
    n = len(rows)
    chr_ = np.tile(np.array(names, np.int32), n)
    pos = np.array([v for r in rows for v in (r[0], r[1])], dtype=np.uint64)
    length = np.array([v for r in rows for v in (r[2], r[3])], dtype=np.uint64)
    return chr_, pos, length, np.full(n, flag, np.uint8)


def random_case(rng, n, n_names=2, span=600, flags=(0, 1, 2, 3)):
    """Anchors near one diagonal per orientation (the right start follows the left one, or runs against it), so that
    links are common."""
    chr_ = rng.integers(0, n_names, 2 * n).astype(np.int32)
    fl = rng.choice(flags, n).astype(np.uint8)
    pl = rng.integers(0, span, n)
    pr = np.where(fl & 1, span + 40 - pl, pl + 40) + rng.integers(-25, 26, n)
    pos = np.column_stack([pl, pr]).reshape(-1).astype(np.uint64)
    length = rng.integers(1, 120, 2 * n).astype(np.uint64)
    return chr_, pos, length, fl


# ---- a brute force of its own: the rule's link written from the signed dl and dr, all paths enumerated ----------------
def brute_link(a, b, rev, max_gap):
    (pl_j, pr_j, ll_j, rl_j), (pl_i, pr_i, ll_i, rl_i) = a, b
    if pl_i <= pl_j or pl_i + ll_i <= pl_j + ll_j:
        return None
    if rev:
        if pr_i >= pr_j or pr_i + rl_i >= pr_j + rl_j:
            return None
        dr = pr_j - (pr_i + rl_i)
    else:
        if pr_i <= pr_j or pr_i + rl_i <= pr_j + rl_j:
            return None
        dr = pr_i - (pr_j + rl_j)
    dl = pl_i - (pl_j + ll_j)
    if max(dl, 0) > max_gap or max(dr, 0) > max_gap:
        return None
    return min(ll_i + min(dl, 0), rl_i + min(dr, 0)) - max(dl, dr, 0)


def brute_f(chr_, pos, length, flags, max_gap):
    """f(q) as the best value over ALL increasing link paths that end in q (no window)."""
    n = len(flags)
    rec = [(int(pos[2 * q]), int(pos[2 * q + 1]), int(length[2 * q]), int(length[2 * q + 1])) for q in range(n)]
    key = [(int(chr_[2 * q]), int(chr_[2 * q + 1]), int(flags[q])) for q in range(n)]
    best = [min(r[2], r[3]) for r in rec]
    for size in range(2, n + 1):
        for path in itertools.permutations(range(n), size):
            if any(key[q] != key[path[0]] for q in path):
                continue
            if any((rec[a][0], rec[a][1], a) >= (rec[b][0], rec[b][1], b) for a, b in zip(path, path[1:])):
                continue
            total = min(rec[path[0]][2], rec[path[0]][3])
            for a, b in zip(path, path[1:]):
                t = brute_link(rec[a], rec[b], key[a][2] & 1, max_gap)
                if t is None:
                    break
                total += t
            else:
                best[path[-1]] = max(best[path[-1]], total)
    return best


def test_f_is_the_best_of_all_paths():
    rng = np.random.default_rng(1)
    linked = 0
    for case in range(150):
        n = int(rng.integers(1, 8))
        args = random_case(rng, n, n_names=1, span=300, flags=(0, 1))
        max_gap = int(rng.choice([0, 20, 100, 10_000]))
        c = chain.chain_host(*args, 1, max_gap, lookback=n)
        assert c.f.tolist() == brute_f(*args, max_gap), case
        linked += int((c.pred >= 0).sum())
    assert linked > 30


def chains_of(c):
    offs = c.chain_offsets.tolist()
    return [c.order[offs[k]:offs[k + 1]].tolist() for k in range(c.n_chains)]


def test_the_four_properties_on_random_cases():
    rng = np.random.default_rng(2)
    kept = cut = 0
    for case in range(400):
        n = int(rng.integers(1, 15))
        chr_, pos, length, flags = args = random_case(rng, n, n_names=1, span=900, flags=(0, 3))
        c = chain.chain_host(*args, 1, 300, lookback=int(rng.choice([1, 2, 64])))
        members = chains_of(c)
        assert sorted(q for m in members for q in m) == list(range(n))                      # a partition
        assert [min(m) for m in members] == sorted(min(m) for m in members)                 # the numbering
        for k, m in enumerate(members):
            assert all(pos[2 * a] < pos[2 * b] for a, b in zip(m, m[1:]))                   # pl strictly increases
            assert c.link[m[0]] == -1 and all(c.link[b] == a for a, b in zip(m, m[1:]))
            assert all(c.chain[q] == k for q in m)
            if c.pred[m[0]] == -1:
                assert c.chain_score[k] == c.f[m[-1]]                                       # an uncut head: f(tail)
            else:
                cut += 1
        kept += c.n_links
        # the best anchor of every tree hangs on its root by kept links
        root = list(range(n))
        for q in sorted(range(n), key=lambda q: (int(flags[q]), int(pos[2 * q]), int(pos[2 * q + 1]), q)):
            if c.pred[q] >= 0:
                root[q] = root[c.pred[q]]
        for r in set(root):
            tree = [q for q in range(n) if root[q] == r]
            top = max(c.f[q] for q in tree)
            reach = [q for q in tree if c.f[q] == top]
            assert any(c.chain[q] == c.chain[r] for q in reach), case
    assert kept > 300 and cut > 0


def staircase(n, step=100, length=60):
    return [(step * k, step * k, length, length) for k in range(n)]


def test_lookback_binds():
    """Anchor 0 is long, those between are tiny and cannot carry its score: the last anchor links to anchor 0 exactly when
    it lies within H ranks."""
    for H in (1, 5, 64):
        for back, links in ((H, True), (H + 1, False)):
            rows = [(0, 0, 5000, 5000)] + [(5000 + k, 4000 - k, 1, 1) for k in range(back - 1)] + [(6000, 6000, 50, 50)]
            c = chain.chain_host(*anchors(rows), 1, 10_000, lookback=H)
            assert (c.pred[back] == 0) == links, (H, back)
            assert c.f[back] == (5000 + 50 - 1000 if links else 50)


def branch_rows():
    """J -> I (small) -> T (huge) beside J -> I' (medium): the second worked example of the header."""
    return [(0, 0, 100, 100), (100, 100, 10, 10), (100, 130, 50, 50), (200, 120, 1000, 1000)]


def test_the_branch_goes_to_the_larger_g_not_the_larger_f():
    c = chain.chain_host(*anchors(branch_rows()), 1, 10_000, 64)
    assert c.f.tolist() == [100, 110, 120, 1020] and c.pred.tolist() == [-1, 0, 0, 1]
    assert c.link.tolist() == [-1, 0, -1, 1]                      # succ(J) = I, and I' is cut off
    assert chains_of(c) == [[0, 1, 3], [2]] and c.chain_score.tolist() == [1020, 50]
    assert c.n_links == 2 and int((c.pred >= 0).sum()) == 3       # one link was cut


def test_a_g_tie_goes_to_the_smaller_rank_and_an_f_tie_to_the_nearer_anchor():
    # two children of J with equal g: the one of the smaller rank stays
    rows = [(0, 0, 100, 100), (100, 100, 20, 20), (100, 130, 50, 50)]    # J -> I: 120; J -> I': 100 + 50 - 30 = 120
    c = chain.chain_host(*anchors(rows), 1, 10_000, 64)
    assert c.f.tolist() == [100, 120, 120] and c.pred.tolist() == [-1, 0, 0] and c.link.tolist() == [-1, 0, -1]
    # two predecessors of K with equal f + t that cannot link each other (pr falls, el stands): the nearer one is taken
    rows = [(0, 10, 190, 180), (10, 0, 180, 190), (200, 200, 500, 500)]   # both -> K: 180 + 500 - 10
    c = chain.chain_host(*anchors(rows), 1, 10_000, 64)
    assert c.f.tolist() == [180, 180, 670] and c.pred.tolist() == [-1, -1, 1]
    assert chains_of(c) == [[0], [1, 2]]


def worked_result():
    """Five duplications in two families: three direct pieces of one pair on (a, b), one unrelated, two reversed pieces."""
    names = ["a", "b"]
    chr_ = [(0, 1)] * 3 + [(0, 0)] + [(0, 1)] * 2
    pos = [(100, 5000), (800, 5650), (1050, 5900), (3000, 9000), (100, 7000), (700, 6500)]
    arm = [(400, 400), (300, 320), (200, 200), (50, 60), (400, 400), (300, 300)]
    flags = [0, 0, 0, 0, 3, 3]
    base = np.array([0, 10_000], np.uint64)
    chr_, pos, arm = np.array(chr_, np.int32), np.array(pos, np.uint64), np.array(arm, np.uint64)
    return sl.ResultArrays("r.fa", 20_000, dict(SETTINGS), names, [0, 1], [0, 10_000], [10_000, 10_000], [0, 2, 2, 6],
                           np.column_stack([base[chr_] + pos, arm]), flags, chr_, pos, np.full(6, 0.5, np.float32))


def test_the_chained_result_and_the_tsv_of_a_worked_example():
    a = worked_result()
    c = chain.Chains.from_arrays(a, host=True)
    assert chains_of(c) == [[0, 1, 2], [3], [4, 5]] and c.chain_score.tolist() == [530, 50, 400 + 300 - 200]
    b = c.to_arrays(a)
    assert b.offs.tolist() == [0, 1, 3]                           # the empty family is gone
    assert b.chr_pos.tolist() == [[100, 5000], [3000, 9000], [100, 6500]]
    assert b.sds.tolist() == [[100, 15_000, 1150, 1100], [3000, 9000, 50, 60], [100, 16_500, 900, 900]]
    assert b.flags.tolist() == [0, 0, 3] and b.identity.tolist() == [0.0] * 3 and b.chr.tolist() == [[0, 1], [0, 0], [0, 1]]
    assert b.settings == a.settings and b.names == a.names and b.strand_name == "r.fa"
    sds, flags = c.proto(a)
    assert sds.dtype == np.uint64 and sds.shape == (3, 4) and flags.dtype == np.uint8
    assert chain.chains_text(a, c) == chain.CHAINS_HEADER + (
        "a\t100\t1250\tb\t5000\t6100\tchain0\t3\t+\t0\t530\t850\t850\n"
        "a\t3000\t3050\ta\t9000\t9060\tchain1\t1\t+\t1\t50\t50\t60\n"
        "a\t100\t1000\tb\t6500\t7400\tchain2\t2\t-\t1\t500\t700\t700\n")
    back = sl.ResultArrays.from_result(sl.parse_result(sl.export_arrays(b, "json")))
    assert (back.sds == b.sds).all() and (back.offs == b.offs).all()


def test_refusals():
    chr_, pos, length, flags = anchors(staircase(3))

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            chain.chain_host(*args, **kw)

    bad = chr_.copy()
    bad[3] = 1
    refused(r"duplication 1 \(right\) has the name id 1, outside \[0, 1\)", bad, pos, length, flags, 1)
    empty = length.copy()
    empty[4] = 0
    refused(r"duplication 2 \(left\) has length 0", chr_, pos, empty, flags, 1)
    top = pos.copy()
    top[1] = M64
    refused(r"duplication 0 \(right\): position 18446744073709551615 \+ length 60 wraps", chr_, top, length, flags, 1)
    long_ = length.copy()
    long_[0] = 2 ** 32
    refused(r"duplication 0 \(left\) has 4294967296 bases", chr_, pos, long_, flags, 1)
    refused("duplication 1 has the flag byte 4, above 3", chr_, pos, length, np.array([0, 4, 0], np.uint8), 1)
    refused("lookback 0 is outside", chr_, pos, length, flags, 1, lookback=0)
    refused("lookback 1025 is outside", chr_, pos, length, flags, 1, lookback=1025)
    refused("max_gap .* is 2\\^62 or more", chr_, pos, length, flags, 1, max_gap=2 ** 62)
    refused("differ in length", chr_, pos, length, flags[:2], 1)
    assert chain.chain_host(chr_, pos, length, flags, 1, 2 ** 62 - 1, 1024).n_chains == 1
    none = chain.chain_host(chr_[:0], pos[:0], length[:0], flags[:0], 4)
    assert none.n_chains == 0 and none.chain_offsets.tolist() == [0] and none.f.dtype == np.int64
    a = worked_result()
    a.names[1] = sl.COLLAPSED_NAME
    with pytest.raises(ValueError, match="the result is collapsed"):
        chain.refuse_collapsed(a)
