"""The tail rule of the placement (asgart_index_set_tail_up; place_tier in asgart_amd/csrc/place_dev.hpp): a segment that
its arm bound sends to tier 2, 4 or 5 and that has at least the tier's threshold of hits runs in the next arm-resident
workgroup tier that holds more.  Placement never changes results: every battery case and two flat tandem arrays (one whose
arm bound fits tier 4, one tier 5) give the oracle's families, ProtoSDs and the same keys with the rule off and on, as single
calls and as one passes call; the array's segment changes tier exactly at its threshold (the per-tier segment counts say
so); forcing every segment into tier 6 leaves nothing to move; a moved segment is still cut into ranges; and the hardware
queue budget (fresh child processes, tests/tail_up_child.py) changes nothing.  Run with `pytest -m gpu` on an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import asgart_amd
import oracle
from asgart_amd import prep, synth
from test_gpu_parity import BATTERY, _battery_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ORIENTATIONS = ((False, False), (True, True))
CHILD_LIMIT_S = 300

# One flat array of 171-bp monomers in 150 kb of background (make_genome's satellite arrays), direct orientation: its
# richest segment has an arm bound of 901 (tier 4 holds 1024, tier 2 512) / 1404 (tier 5 holds 2048) and about 2 200
# processed probes -- far below option long3, so its bound alone places it.  `up`: where the rule sends it.
ARRAYS = {
    "array_tier4": dict(copies=130, tier=4, up=5, bound=(513, 1024)),
    "array_tier5": dict(copies=200, tier=5, up=6, bound=(1025, 2048)),
}
_CASES = {}
# the battery cases with a young high-copy repeat family (15-35 % of the text at up to 5 % divergence: tens to hundreds of
# hits per probe): their segments reach tiers 2, 4 and 5, and with the rule on at 64 hits some must move.  The other cases
# place nothing there (their segments fit one wave), so for them the rule has nothing to do; the array cases below cover
# the moves tier by tier.
MOVES_AT_64 = {"card_skip", "dense_repeats", "k31_odd", "k42"}


def walk_segments(status, counts, tstar):
    """The placement walk over one chunk's probes (seg_stats_kernel): [(hits, arm bound, processed probes)] of its
    segments.  A segment starts at a hit-probe and ends with the t*-th quiet probe in a row; skipped probes (status != 0)
    neither count nor interrupt; the bound is the largest hit total of t* + 1 consecutive processed probes."""
    out, i, n = [], 0, len(counts)
    while i < n:
        if status[i] != 0 or counts[i] == 0:
            i += 1
            continue
        quiet, ring, total, bound, n_proc, j = 0, [], 0, 0, 0, i
        while j < n:
            if status[j] == 0:
                v = int(counts[j])
                quiet = quiet + 1 if v == 0 else 0
                if quiet >= tstar:
                    break
                n_proc += 1
                ring = (ring + [v])[-(min(tstar, 64) + 1):]
                bound = max(bound, sum(ring))
                total += v
            j += 1
        out.append((total, bound, n_proc))
        i = j + 1
    return out


def array_case(name):
    """-> (prepared records, oracle index, expected results per orientation, hits of the array's segment)"""
    if name not in _CASES:
        spec = ARRAYS[name]
        recs = synth.make_genome([150_000], seed=1, sd_per_mb=0, alu_frac=0.0, l1_frac=0.0, sat_per_record=1,
                                 sat_copies=(spec["copies"], spec["copies"] + 1), gaps=False, short_n_per_mb=0.0)
        pr = prep.prepare_records(recs)
        assert len(pr.data) <= 200_000
        oidx = oracle.Index.build(pr.data)
        exp = [oidx.run_raw(pr.chunks, oracle.make_settings(reverse=r, complement=c), threads=4) for r, c in ORIENTATIONS]
        ost = oracle.make_settings()
        st = asgart_amd.RunSettings.from_cli()
        step = st.probe_size // 2
        segs = []
        for ch in pr.chunks:
            status, offs, _ = oidx.probe_hits(oracle.prepare_needle(pr.data, ch, ost), ch[0], ost)
            segs += walk_segments(status, np.diff(offs.astype(np.int64)), max(1, (st.max_gap_size + step - 1) // step))
        segs.sort(reverse=True)
        (hits, bound, n_proc), second = segs[0], segs[1]
        assert spec["bound"][0] <= bound <= spec["bound"][1], (name, bound)   # the tier its bound gives it
        assert n_proc < 16384 and second[0] < hits - 1, (name, segs[:2])     # not a long3 segment; no other as rich
        _CASES[name] = (pr, oidx, exp, hits)
    return _CASES[name]


def _settings(cli=None):
    return [asgart_amd.RunSettings.from_cli(reverse=r, complement=c, **(cli or {})) for r, c in ORIENTATIONS]


def run_all(idx, chunks, sts):
    """Both orientations as single calls and as one passes call, with keys: [(offsets, sds, keys)] x 4 and the per-tier
    segment counts of the direct single call and of the passes call."""
    out, tiers = [], []
    for i, st in enumerate(sts):
        out.append(idx.search_duplications_raw(chunks, st, with_keys=True))
        if i == 0:
            tiers.append(idx.tier_segments())
    out += idx.search_duplications_passes(chunks, sts, with_keys=True)
    tiers.append(idx.tier_segments())
    return out, tiers


def check_against(got, exp, ref, tag):
    for j, (g, e) in enumerate(zip(got, exp + exp)):
        assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]), \
            (tag, j, f"{len(g[0]) - 1} families / {len(g[1])} ProtoSDs, oracle {len(e[0]) - 1} / {len(e[1])}")
        if ref is not None:
            assert np.array_equal(g[2], ref[j][2]), (tag, j, "keys")


def digest(results):
    h = hashlib.sha256()
    for r in results:
        for a in r:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", sorted(BATTERY))
def test_battery_results_do_not_depend_on_the_tail_rule(hiplib, name):
    """Rule off, rule on with a threshold of 64 hits (most segments with arms to speak of move up a tier), and the same
    with every multi-hit segment forced into tier 6."""
    pr, cli = _battery_case(name)
    oidx = oracle.Index.build(pr.data)
    exp = [oidx.run_raw(pr.chunks, oracle.make_settings(reverse=r, complement=c, **cli), threads=4) for r, c in ORIENTATIONS]
    sts = _settings(cli)
    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        idx.set_option("fuse_passes", 2)   # (the passes call always as ONE job: its tier counts are the job's)
        idx.set_tail_up(0)
        ref, _ = run_all(idx, pr.chunks, sts)
        check_against(ref, exp, None, (name, "off"))
        idx.set_tail_up(2, 64)
        got, tiers = run_all(idx, pr.chunks, sts)
        check_against(got, exp, ref, (name, "on, 64 hits"))
        print(f"{name}: segments moved at 64 hits (single call, passes call): {[m for _, m in tiers]}")
        if name in MOVES_AT_64:
            assert all(m > 0 for _, m in tiers), (name, tiers)
        idx.set_option("force_tier", 6)
        got, forced = run_all(idx, pr.chunks, sts)
        check_against(got, exp, ref, (name, "on, 64 hits, force_tier 6"))
        idx.set_tail_up(0)
        got, forced_off = run_all(idx, pr.chunks, sts)
        check_against(got, exp, ref, (name, "off, force_tier 6"))
        for (n_on, _), (n_off, _) in zip(forced, forced_off):
            assert np.array_equal(n_on, n_off), (name, "force_tier 6", n_on, n_off)


@pytest.mark.parametrize("name", sorted(ARRAYS))
def test_the_array_segment_moves_exactly_at_its_threshold(hiplib, name):
    spec = ARRAYS[name]
    pr, oidx, exp, hits = array_case(name)
    sts = _settings()
    t, up = spec["tier"] - 1, spec["up"] - 1
    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        idx.set_option("fuse_passes", 2)   # (the passes call always as ONE job: its tier counts are the job's)
        idx.set_tail_up(0)
        ref, base = run_all(idx, pr.chunks, sts)
        check_against(ref, exp, None, (name, "off"))
        assert all(n[t] >= 1 and moved == 0 for n, moved in base), (name, base)
        for thr, moves in ((hits + 1, False), (hits, True), (hits - 1, True)):   # the segment has thr - 1, thr, thr + 1 hits
            idx.set_tail_up(2, thr)
            got, tiers = run_all(idx, pr.chunks, sts)
            check_against(got, exp, ref, (name, thr))
            for (n, moved), (n0, _) in zip(tiers, base):
                delta = n.astype(np.int64) - n0.astype(np.int64)
                want = np.zeros(7, dtype=np.int64)
                if moves:
                    want[t], want[up] = -1, 1
                assert moved == (1 if moves else 0) and np.array_equal(delta, want), (name, thr, hits, n0, n, moved)
        # every multi-hit segment forced into tier 6: the rule has nothing left to change
        idx.set_option("force_tier", 6)
        idx.set_tail_up(2, hits)
        got, forced = run_all(idx, pr.chunks, sts)
        check_against(got, exp, ref, (name, "force_tier 6, on"))
        idx.set_tail_up(0)
        got, forced_off = run_all(idx, pr.chunks, sts)
        check_against(got, exp, ref, (name, "force_tier 6, off"))
        for (n_on, _), (n_off, _) in zip(forced, forced_off):
            assert np.array_equal(n_on, n_off) and n_on[t] == 0, (name, n_on, n_off)


@pytest.mark.parametrize("name", sorted(ARRAYS))
def test_a_moved_segment_is_still_cut_into_ranges(hiplib, name):
    """Ranges of 256 probes (the array's segment spans 2 200): the cut planner reads the tier the rule chose, the ranges
    run and join up to the oracle's result."""
    pr, oidx, exp, hits = array_case(name)
    sts = _settings()
    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        for a, v in (("split", 1), ("split_len", 256), ("split_warm", 256), ("split_min", 0)):
            idx.set_option(a, v)
        cut = []
        for mode in (0, 2):
            idx.set_tail_up(mode, hits)
            got = idx.search_duplications_raw(pr.chunks, sts[0], with_keys=True)
            s, (_, moved) = idx.stats(0), idx.tier_segments()
            assert np.array_equal(got[0], exp[0][0]) and np.array_equal(got[1], exp[0][1]), (name, mode)
            assert s.split_segments >= 1 and moved == (1 if mode else 0), (name, mode, s.split_segments, moved)
            cut.append((int(s.split_segments), digest([got])))
        assert cut[0] == cut[1], (name, cut)


def _child(budget):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASGART_")}   # shipped defaults, no presets
    env["GPU_MAX_HW_QUEUES"] = str(budget)
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(HERE, "tail_up_child.py")],
                       env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S + 60)
    tail = f"exit {p.returncode}\n--- stdout\n{p.stdout[-3000:]}\n--- stderr\n{p.stderr[-3000:]}"
    assert p.returncode == 0, tail
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, tail
    return json.loads(lines[0]), p.stderr, tail


def test_the_array_cases_do_not_depend_on_the_queue_budget(hiplib):
    """Budgets 2, 4 and 8, a fresh process each: the same families, ProtoSDs and keys, rule off, on and in its shipped
    default mode, which is on with 2 and 4 queues (fewer tier streams than the five arm-resident tiers) and off with 8 (six
    tier streams)."""
    out = {}
    for budget in (2, 4, 8):
        res, err, tail = _child(budget)
        assert f"tier plan ({min(6, budget)} tier streams" in err, tail
        out[budget] = res
    for name in ARRAYS:
        for budget, res in out.items():
            r = res[name]
            assert r["off"]["digest"] == r["on"]["digest"] == r["default"]["digest"] == out[2][name]["off"]["digest"], (name, budget)
            assert r["off"]["moved"] == [0, 0] and r["on"]["moved"] == [1, 1], (name, budget, r)
            assert r["default"]["moved"] == ([1, 1] if budget < 5 else [0, 0]), (name, budget, r)
            assert r["off"]["tiers"] == out[2][name]["off"]["tiers"] and r["on"]["tiers"] == out[2][name]["on"]["tiers"], (name, budget)
            assert r["default"]["tiers"] == r["on" if budget < 5 else "off"]["tiers"], (name, budget, r)
