"""The header's promise for asgart_index_set_option -- RESULTS NEVER DEPEND ON ANY OF THEM -- held against the CPU
oracle: every value of the sweep table (tests/option_sweep.py) on the battery cases in every orientation, seeded random
combinations of them, one long-lived index answering a sequence of different calls, and the full-size digests with the
shipped defaults over the first three calls of one index (what bench.py times is the 2nd ... Nth).  Run with
`pytest -m gpu` on an MI355X."""
import os

import numpy as np
import pytest

import asgart_amd
import option_sweep as osw
import oracle
from asgart_amd import prep, synth
from test_gpu_parity import MODES, _battery_case, _sha_slabs

pytestmark = pytest.mark.gpu

SWEEP_CASES = ["dense_repeats", "satellites", "long_sds", "k12", "k31_odd", "masked"]

# the statistics that describe the RESULT of a search call: they must not move with options or with what an index has
# learned from its earlier calls
RESULT_COUNTERS = ("probes_total", "probes_n_skipped", "probes_searched", "probes_card_skipped", "probes_with_hits",
                   "raw_hits", "filtered_hits", "segments", "families", "proto_sds")


def _shipped_defaults(monkeypatch):
    """No option preset through ASGART_<NAME> (tests/conftest.py presets lazy_aux = 0): an index created now runs the
    shipped defaults."""
    for name in osw.DEFAULTS:
        monkeypatch.delenv(f"ASGART_{name.upper()}", raising=False)


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def _what(got, exp):
    return f"{len(got[0]) - 1} families / {len(got[1])} ProtoSDs, oracle {len(exp[0]) - 1} / {len(exp[1])}"


def _sharded(idx, chunks, st, R=3):
    return asgart_amd.merge_shards([idx.search_duplications_raw(chunks, st, shard=r, n_shards=R, with_keys=True)
                                    for r in range(R)])


def _run_form(idx, form, chunks, sts, exp, tag, failures):
    """The call form an entry affects, in every orientation; a mismatch is recorded with `tag`, an error raised."""
    if form == "single":
        for m in MODES:
            got = idx.search_duplications_raw(chunks, sts[m])
            if not _same(got, exp[m]):
                failures.append(f"{tag} {m}: {_what(got, exp[m])}")
    elif form == "sharded":
        for m in MODES:
            got = _sharded(idx, chunks, sts[m])
            if not _same(got, exp[m]):
                failures.append(f"{tag} {m} 3 shards: {_what(got, exp[m])}")
    else:
        # the passes call: three in a row (fuse_passes = 1 times the two ways on the calls after the first)
        for rep in range(3):
            for m, got in zip(MODES, idx.search_duplications_passes(chunks, [sts[m] for m in MODES])):
                if not _same(got, exp[m]):
                    failures.append(f"{tag} {m} passes call {rep}: {_what(got, exp[m])}")


def _apply(idx, sets):
    for a, v in sets.items():
        idx.set_option(a, v)


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_every_option_value_gives_the_oracle_result(hiplib, name, monkeypatch):
    """One option at a time (plus the options it only acts together with), every value of the sweep table, on one
    battery case in all four orientations: bit-exact with the oracle, whose result is computed once per orientation --
    by the header's promise it cannot depend on the options.  Options read at creation run on a fresh index that sorts
    its own suffixes; the others on one index per case, reset to the defaults after every entry."""
    _shipped_defaults(monkeypatch)
    pr, cli = _battery_case(name)
    k = cli.get("k", 20)
    oidx = oracle.Index.build(pr.data)
    sts = {m: asgart_amd.RunSettings.from_cli(reverse=m[0], complement=m[1], **cli) for m in MODES}
    exp = {m: oidx.run_raw(pr.chunks, oracle.make_settings(reverse=m[0], complement=m[1], **cli), threads=4) for m in MODES}
    failures = []
    with asgart_amd.Index(pr.data, oidx.sa) as shared:
        for opt, o in osw.entries():
            tag = f"{name}: {osw.describe(opt, o)}"
            env = {a: osw.resolve(v, k) for a, v in o.env.items()}
            sets = dict(o.with_)
            if opt not in env:
                sets[opt] = osw.resolve(o.value, k)
            if not env:
                try:
                    _apply(shared, sets)
                    _run_form(shared, o.form, pr.chunks, sts, exp, tag, failures)
                finally:
                    _apply(shared, {a: osw.DEFAULTS[a] for a in sets})
                continue
            for a, v in env.items():
                monkeypatch.setenv(f"ASGART_{a.upper()}", str(v))
            try:
                with asgart_amd.Index(pr.data, None) as idx:
                    assert np.array_equal(idx.sa_read(0, len(pr.data)), oidx.sa), tag
                    _apply(idx, sets)
                    _run_form(idx, o.form, pr.chunks, sts, exp, tag, failures)
            finally:
                for a in env:
                    monkeypatch.delenv(f"ASGART_{a.upper()}")
    assert not failures, "\n".join(failures)


def _random_genome(rng):
    """A genome and settings shaped like test_random_sweep_default_and_forced_tiers."""
    lens = [int(x) for x in rng.integers(60_000, 220_000, size=int(rng.integers(1, 4)))]
    gen = dict(sd_per_mb=float(rng.uniform(5, 60)), sd_len=(500, int(rng.integers(2_000, 40_000))),
               alu_frac=float(rng.uniform(0.0, 0.3)), l1_frac=float(rng.uniform(0.0, 0.05)),
               sat_per_record=int(rng.integers(0, 3)), sat_copies=(20, int(rng.integers(60, 500))),
               alu_div=(0.005, float(rng.uniform(0.03, 0.15))))
    recs = synth.make_genome(lens, seed=int(rng.integers(1, 1 << 30)), **gen)
    pr = prep.prepare_records(recs, skip_masked=bool(rng.integers(0, 2)))
    cli = dict(k=int(rng.choice([10, 12, 16, 20, 21, 25])), gap=int(rng.choice([0, 30, 100, 250])),
               min_length=int(rng.choice([100, 300, 1000])), max_cardinality=int(rng.choice([30, 200, 500, 1500])))
    return pr, cli


@pytest.mark.parametrize("seed", range(12))
def test_random_option_combinations(hiplib, seed, monkeypatch):
    """Several options of the table at once, drawn by the seed, on a random genome with random settings: single calls
    in two orientations, both as one passes call (three times) and both over 3 shards merged by key -- all equal to the
    oracle.  Every message names the seed and the option vector (environment presets first)."""
    _shipped_defaults(monkeypatch)
    rng = np.random.default_rng(7100 + seed)
    pr, cli = _random_genome(rng)
    k = cli["k"]
    table = [(n, o) for n, o in osw.entries() if not o.env]
    vec = {}
    for j in rng.choice(len(table), size=int(rng.integers(3, 7)), replace=False):
        opt, o = table[int(j)]
        vec.update(o.with_)
        vec[opt] = osw.resolve(o.value, k)
    env = {}
    if rng.integers(0, 3) == 0:
        env["force_wide"] = 1
    if rng.integers(0, 3) == 0:
        env["ptab_depth"] = int(rng.choice([1, 2, min(k - 1, 15), min(k, 15), 15]))
    for a, v in env.items():
        monkeypatch.setenv(f"ASGART_{a.upper()}", str(v))
    tag = f"seed {seed}: env {env} options {vec} settings {cli}"
    modes = [(False, False), (True, True)] if rng.integers(0, 2) else [(True, False), (False, True)]
    oidx = oracle.Index.build(pr.data)
    exp = {m: oidx.run_raw(pr.chunks, oracle.make_settings(reverse=m[0], complement=m[1], **cli), threads=4) for m in modes}
    sts = {m: asgart_amd.RunSettings.from_cli(reverse=m[0], complement=m[1], **cli) for m in modes}
    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        _apply(idx, vec)
        for m in modes:
            got = idx.search_duplications_raw(pr.chunks, sts[m])
            assert _same(got, exp[m]), (tag, m, _what(got, exp[m]))
        for rep in range(3):
            for m, got in zip(modes, idx.search_duplications_passes(pr.chunks, [sts[m] for m in modes])):
                assert _same(got, exp[m]), (tag, m, "passes call", rep, _what(got, exp[m]))
        for m in modes:
            got = _sharded(idx, pr.chunks, sts[m])
            assert _same(got, exp[m]), (tag, m, "3 shards", _what(got, exp[m]))


# the sequence of calls of test_one_index_many_calls: (form, orientations, settings, chunk list, options set before it)
_DD, _RC, _R, _C = (False, False), (True, True), (True, False), (False, True)
_CUT = dict(long3=256, split_len=64, split_warm=1, split_min=0, split_warm_max=1 << 22)
_UNCUT = dict(long3=16384, split_len=0, split_warm=6144, split_warm_max=65536)
_K20 = dict(k=20, gap=100, min_length=300)
_K12 = dict(k=12, gap=50, min_length=300)
_K16 = dict(k=16, gap=0, min_length=200)
CALLS = [
    ("single", [_DD], _K20, "all", {}),
    ("single", [_RC], _K20, "all", {}),                 # (the second call builds the position-sorted lists)
    ("passes", [_DD, _RC], _K20, "all", {}),
    ("single", [_R], _K20, "shifted", {}),
    ("single", [_C], _K12, "all", {}),                  # another k: index_prepare again
    ("single", [_DD], dict(_K12, gap=30), "all", {}),
    ("sharded", [_RC], _K12, "all", {}),
    ("single", [_DD], _K20, "all", {}),                 # back to k = 20
    ("single", [_DD], _K20, "all", {"posbits": 0}),
    ("single", [_DD], _K20, "all", {"posbits": 1}),
    ("single", [_RC], dict(_K20, min_length=1000, max_cardinality=40), "all", {}),
    ("single", [_DD], _K20, "all", _CUT),               # ranges of 64 probes with 1 probe of warm-up: cuts fail ...
    ("single", [_DD], _K20, "all", {}),                 # ... and the next call starts from split_blocked
    ("single", [_RC], _K20, "all", {}),
    ("passes", [_DD, _RC], _K20, "all", {}),
    ("single", [_DD], _K20, "all", {"split_len": 65, "split_warm": 0}),
    ("sharded", [_DD], _K20, "all", {}),
    ("single", [_DD], _K20, "all", _UNCUT),
    ("single", [_C], _K16, "all", {}),
    ("passes", [_DD, _R, _C, _RC], _K16, "all", {}),
    ("single", [_DD], _K20, "halves", {}),
    ("single", [_DD], dict(_K20, max_cardinality=200), "all", {}),
    ("sharded_passes", [_DD, _RC], _K20, "all", {"shard_lookback": 1, "shard_lookahead": 1}),
    ("passes", [_DD, _RC], _K20, "all", {"fuse_passes": 2}),
    ("passes", [_DD, _RC], _K20, "all", {"fuse_passes": 0}),
    ("passes", [_DD, _RC], _K20, "all", {"fuse_passes": 1, "shard_lookback": 4096, "shard_lookahead": 0}),
    ("single", [_R], _K12, "shifted", {}),
    ("single", [_DD], _K20, "all", {"posbits": 0}),
    ("single", [_RC], dict(_K20, gap=250, min_length=100), "all", {"posbits": 1}),
    ("passes", [_DD, _RC], _K20, "all", {}),
]


def test_one_index_many_calls(hiplib, monkeypatch):
    """One index, shipped defaults, answering the calls of CALLS in turn -- orientation, k (and back), gap, minimum
    length and cardinality, chunk lists, shard windows, single and passes calls, position bits off and on, cuts that
    fail (split_blocked) -- every result equal to the oracle's run of that call.  What the index learns between calls
    may only change the work it does: a call made again reports the same RESULT_COUNTERS, and every single call's
    family and ProtoSD counters are its result's."""
    _shipped_defaults(monkeypatch)
    recs = synth.make_genome([260_000, 140_000], seed=41, sd_per_mb=30, sd_len=(1000, 20_000), alu_frac=0.2,
                             alu_div=(0.005, 0.05), l1_frac=0.0, sat_per_record=2, sat_copies=(50, 300))
    pr = prep.prepare_records(recs, skip_masked=False)
    lists = {"all": list(pr.chunks),
             "shifted": [(s0 + 3, l0 - 7) for s0, l0 in pr.chunks if l0 > 2000],
             "halves": [c for s0, l0 in pr.chunks if l0 > 4000
                        for c in ((s0, l0 // 2 + 11), (s0 + l0 // 2 - 5, l0 - l0 // 2 + 5))]}
    oidx = oracle.Index.build(pr.data)
    expected, counters = {}, {}
    refused = 0

    def oracle_run(chunks_name, cli, m):
        key = (chunks_name, tuple(sorted(cli.items())), m)
        if key not in expected:
            expected[key] = oidx.run_raw(lists[chunks_name], oracle.make_settings(reverse=m[0], complement=m[1], **cli),
                                         threads=4)
        return expected[key]

    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        for i, (form, modes, cli, chunks_name, opts) in enumerate(CALLS):
            _apply(idx, opts)
            tag = (i, form, modes, cli, chunks_name, opts)
            chunks = lists[chunks_name]
            sts = [asgart_amd.RunSettings.from_cli(reverse=m[0], complement=m[1], **cli) for m in modes]
            if form == "single":
                got = [idx.search_duplications_raw(chunks, sts[0])]
                stt = idx.stats().as_dict()
                refused += stt["split_refused"]
                assert (stt["families"], stt["proto_sds"]) == (len(got[0][0]) - 1, len(got[0][1])), tag
                key = (chunks_name, tuple(sorted(cli.items())), modes[0])
                seen = counters.setdefault(key, {c: stt[c] for c in RESULT_COUNTERS})
                for c in RESULT_COUNTERS:
                    assert stt[c] == seen[c], (tag, c, stt[c], seen[c])
            elif form == "sharded":
                got = [_sharded(idx, chunks, sts[0])]
            elif form == "passes":
                got = idx.search_duplications_passes(chunks, sts)
            else:
                parts = [idx.search_duplications_passes(chunks, sts, shard=r, n_shards=3, with_keys=True) for r in range(3)]
                got = [asgart_amd.merge_shards([p[j] for p in parts]) for j in range(len(modes))]
            for m, g in zip(modes, got):
                e = oracle_run(chunks_name, cli, m)
                assert _same(g, e), (tag, m, _what(g, e))
    assert refused > 0, "no cut failed: split_blocked was never filled"


# digest counters that are not results: none of the digests' counters is exempt today; these are the ones that would be
EXEMPT_COUNTERS = {
    "probes_filter_rejected": "probes the learned position bits answered: zero in the cold call, more in every later one",
    "split_segments": "segments cut into ranges: the cut plan changes with what split_blocked holds",
    "split_refused": "cuts that did not hold: the next call starts those ranges further in front",
    "search_launches": "launches of the probe search: an implementation count",
    "bisect_steps": "the yardstick's bisection steps, only with the accounting pass",
    "overflow_segments": "segments a tier gave up on: depends on placement, not on the result",
    "heavy_segments": "segments placed in the workgroup tiers",
    "passes": "how the passes call ran: one job or pipelined (fuse_passes = 1 times both ways)",
}


def _check_three_calls_shipped_defaults(name, monkeypatch):
    """The passes call of a digest configuration three times on one index with the shipped defaults (no ASGART_*
    preset: lazy_aux = 1, learned position bits): cold, the call that builds the position-sorted lists, steady state --
    each result hashing to the committed digest of the oracle, each call's result counters equal to the digest's."""
    import json

    _shipped_defaults(monkeypatch)
    with open(os.path.join(os.path.dirname(__file__), "golden", "digests.json")) as fh:
        d = json.load(fh)[name]
    recs = synth.config_genome(d["synth_config"], d["scale"])
    pr = prep.prepare_records(recs, skip_masked=d["skip_masked"])
    del recs
    assert len(pr.data) == d["text_bytes"] and len(pr.chunks) == d["chunks"]
    assert _sha_slabs([np.array(pr.chunks, dtype=np.uint64)], "<u8") == d["chunks_sha256"]
    cli = d["settings"]
    wants = list(d["passes"].values())
    assert len(wants) == 2, name
    sts = [asgart_amd.RunSettings.from_cli(k=cli["k"], gap=cli["gap"], min_length=cli["min_length"],
                                           max_cardinality=cli["max_cardinality"], reverse=w["reverse"],
                                           complement=w["complement"]) for w in wants]
    compared = [c for c in wants[0]["counters"] if c not in EXEMPT_COUNTERS]
    assert compared, name
    rejected = []
    with asgart_amd.Index(pr.data, None) as idx:
        for call in ("cold", "builds the lists", "steady"):
            got = idx.search_duplications_passes(pr.chunks, sts)
            for w, (offs, sds) in zip(wants, got):
                assert (len(offs) - 1, len(sds)) == (w["n_families"], w["n_sds"]), (name, call)
                assert _sha_slabs([offs], "<u8") == w["fam_offsets_sha256"], (name, call)
                assert _sha_slabs([sds], "<u8") == w["sds_sha256"], (name, call)
            stt = idx.stats().as_dict()
            if stt["passes"] == len(wants):   # (one job: the counters are sums over the passes)
                for c in compared:
                    assert stt[c] == sum(w["counters"][c] for w in wants), (name, call, c, stt[c])
            if name == "cfg3s":   # (the accounting pass of stats(1) is not free at GRCh38 size)
                rejected.append(idx.stats(1).probes_filter_rejected)
    assert not rejected or (rejected[0] == 0 and rejected[-1] > 0), (name, rejected)


def test_cfg3s_three_calls_shipped_defaults(hiplib, monkeypatch):
    _check_three_calls_shipped_defaults("cfg3s", monkeypatch)


def test_cfg4_three_calls_shipped_defaults(hiplib, monkeypatch):
    _check_three_calls_shipped_defaults("cfg4", monkeypatch)


@pytest.mark.parametrize("order", [1, 6336, 7777777, 21])
def test_tier_order_that_leaves_tiers_out_still_runs_every_tier(hiplib, order, monkeypatch):
    """Option tier_order accepts any digits 1..7; a tier it did not name used to be never launched (its segments lost:
    tier_order = 7777777 gave no family at all) and a repeated digit launched a tier twice.  Every tier now runs exactly
    once, the named ones first: every segment forced above tier 1 so that all workgroup tiers hold work."""
    _shipped_defaults(monkeypatch)
    pr, cli = _battery_case("dense_repeats")
    oidx = oracle.Index.build(pr.data)
    with asgart_amd.Index(pr.data, oidx.sa) as idx:
        idx.set_option("tier_order", order)
        for force in (0, 2, 6):
            idx.set_option("force_tier", force)
            for m in ((False, False), (True, True)):
                st = asgart_amd.RunSettings.from_cli(reverse=m[0], complement=m[1], **cli)
                exp = oidx.run_raw(pr.chunks, oracle.make_settings(reverse=m[0], complement=m[1], **cli), threads=4)
                got = idx.search_duplications_raw(pr.chunks, st)
                assert _same(got, exp), (order, force, m, _what(got, exp))
