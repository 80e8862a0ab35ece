"""The sweep table of the index options (asgart_index_set_option, include/asgart_hip.h): every option of kOptions
(asgart_amd/csrc/index.hip) and grid1..grid7 either has values to sweep here or is excluded with a reason.  The header
promises that results never depend on any of them; tests/test_gpu_options.py holds the library to that for every value
below, and tests/test_option_table.py fails the CPU suite when an option is added without an entry.

An entry is an `Opt`: the option's value plus, where the option only takes effect together with others, those others
(`with_`), options that must be preset through the environment before the index is created (`env`: ptab_depth,
force_wide and what only the index build reads), and the call form the option affects (`form`: "single" search calls,
"sharded" calls over 3 shards merged by key, or "passes" calls over all four orientations as one request)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Union

Value = Union[int, str]   # str: "k-1" / "k", the probe size of the case (ptab_depth)


@dataclass(frozen=True)
class Opt:
    value: Value
    with_: Dict[str, int] = field(default_factory=dict)
    env: Dict[str, int] = field(default_factory=dict)
    form: str = "single"


# the defaults of struct Options (asgart_amd/csrc/index.hpp); test_option_table.py checks them against the source
DEFAULTS = {
    "shard_lookback": 4096, "shard_lookahead": 0, "force_tier": 0, "arms_kernel": 1, "long3": 16384, "cap1": 256,
    "debug": 0, "test_cap_limit": -1, "test_genbits": 22, "test_k8_delay": 0, "tier_order": 3654217, "ptab_depth": 0,
    "force_wide": 0, "test_wide_batch": 0, "rank_lists": 1, "cap6_pct": 140, "test_fail_alloc": -1, "solo": 1,
    "cap6w_pct": 160, "cap45_pct": 100, "cap3_pct": 160, "posbits": 1, "barren": 2, "fuse_passes": 1, "fuse_pole_pct": 88,
    "lazy_aux": 1, "dense3": 16, "dense6": 32, "split": 1, "split_len": 0, "split_runs": 224, "split_warm": 6144,
    "split_warm_max": 65536, "split_min": 0, "cache_calls": 2, "prewarm": 1, "test_stall_s": 0, "watchdog_s": 120,
    **{f"grid{t}": 0 for t in range(1, 8)},
}

# fixed when the index is created: set through ASGART_<NAME> only
CREATION_ONLY = {"ptab_depth", "force_wide"}

# ranges cut into ranges of a few hundred probes need long segments in the long-shape tiers: long3 = 256 sends every
# segment of 256 probes and more there
_CUTS = {"long3": 256, "split_min": 0}


def _plain(*values, **kw) -> List[Opt]:
    return [Opt(v, **kw) for v in values]


SWEEP: Dict[str, List[Opt]] = {
    # halos of a sharded call, in probes: 1 / 0 force the look-back / look-ahead retries at every shard edge
    "shard_lookback": _plain(1, 2, 4096, 1 << 31, form="sharded"),
    "shard_lookahead": _plain(0, 1, 3, 1 << 31, form="sharded"),
    "force_tier": _plain(0, 1, 2, 3, 4, 5, 6, 7),
    "arms_kernel": _plain(0, 1),
    # long segments to the long-shape tiers: every segment (0 = off, 1 = all), around the default, none
    "long3": _plain(0, 1, 255, 16383, 16384, 16385, 1 << 31),
    "cap1": _plain(1, 2, 64, 255, 256),
    "test_cap_limit": _plain(-1, 2, 24, 100, 1 << 31),
    "test_genbits": _plain(2, 3, 5, 21, 22),
    "test_k8_delay": _plain(0, 2_000) + [Opt(2_000, with_={"force_tier": 3})],
    # permutations, and digit strings that leave tiers out or repeat them (every tier must still run exactly once)
    "tier_order": _plain(3654217, 1234567, 7654321, 2143657, 5674321, 1, 6336, 7777777),
    "ptab_depth": [Opt(0, env={"ptab_depth": 0}), Opt(1, env={"ptab_depth": 1}), Opt(2, env={"ptab_depth": 2}),
                   Opt("k-1", env={"ptab_depth": "k-1"}), Opt("k", env={"ptab_depth": "k"}),
                   Opt(15, env={"ptab_depth": 15})],
    "force_wide": [Opt(0, env={"force_wide": 0}), Opt(1, env={"force_wide": 1})],
    # the 64-bit suffix sorter's batch (read by the build of an index that sorts its own suffixes with 64-bit slots)
    "test_wide_batch": [Opt(v, env={"force_wide": 1, "test_wide_batch": v}) for v in (0, 1000, 1 << 40)],
    "rank_lists": _plain(0, 1),
    "lazy_aux": _plain(0, 1),
    "posbits": _plain(0, 1),
    "fuse_passes": _plain(0, 1, 2, form="passes"),
    "fuse_pole_pct": _plain(1, 87, 88, 89, 1000, form="passes"),
    "barren": _plain(0, 1, 2),
    "dense3": _plain(0, 1, 15, 16, 17, 1 << 20),
    "dense6": _plain(0, 1, 31, 32, 33, 1 << 20),
    "prewarm": _plain(0, 1),
    "cache_calls": _plain(0, 1, 2, 3, 1_000_000),
    # split = 2 cuts with 64-bit positions too: under force_wide; every value also with segments long enough to cut
    "split": _plain(0, 1, 2) + [Opt(2, env={"force_wide": 1}), Opt(1, env={"force_wide": 1}),
                                Opt(2, with_={**_CUTS, "split_len": 128}, env={"force_wide": 1}),
                                Opt(1, with_={**_CUTS, "split_len": 128})],
    # below 64 the ranges are off; 64 and 65 are the shortest ranges, 127 one short of the tandem arrays' shapes
    "split_len": [Opt(v, with_={"split_min": 0}) for v in (0, 63, 64, 65, 127, 2048, 1 << 20)]
                 + [Opt(v, with_=_CUTS) for v in (64, 65, 127, 2048)],
    "split_runs": _plain(1, 2, 223, 224, 225, 3072) + [Opt(v, with_={"long3": 256}) for v in (1, 3072)],
    "split_warm": [Opt(v, with_={**_CUTS, "split_len": 128}) for v in (0, 1, 64, 6144, 1 << 20)] + _plain(0, 1),
    "split_warm_max": [Opt(v, with_={**_CUTS, "split_len": 128, "split_warm": 64}) for v in (0, 1, 65536, 1 << 22)],
    "split_min": [Opt(v, with_={"long3": 256, "split_len": 64}) for v in (0, 1, 256, 1 << 31)],
    "cap6_pct": _plain(100, 139, 140, 141, 200),
    "cap6w_pct": [Opt(v, env={"force_wide": 1}) for v in (100, 159, 160, 161, 400)],
    "cap3_pct": _plain(100, 159, 160, 161, 400),
    "cap45_pct": _plain(100, 101, 800),
    "solo": _plain(0, 1, 2, 16, 17, 47, 48),
    **{f"grid{t}": _plain(0, 1, 1 << 20) for t in range(1, 8)},
}

# options no sweep entry sets, each with the reason
EXCLUDED = {
    "debug": "diagnostics on stderr only; results under it are not a tuning question",
    "watchdog_s": "a time limit; test_watchdog_gives_up_on_a_stalled_device_and_names_the_phase covers it",
    "test_stall_s": "stalls the device on purpose; the watchdog test covers it",
    "test_fail_alloc": "makes an allocation fail on purpose; test_out_of_memory_paths_release_what_they_hold covers it",
}

# an end of an option's range that the sweep leaves out, with the reason (every other option sweeps lo and hi)
ENDS_NOT_SWEPT = {
    ("test_k8_delay", "hi"): "2^22 cycles in every K8 step turn one call into minutes; 2 000 cycles already outlast the "
                             "arm waves (test_k8_free_counts_do_not_depend_on_timing)",
}


def resolve(v: Value, k: int) -> int:
    """A symbolic value for a case of probe size k (ptab_depth: at most 15)."""
    if v == "k-1":
        return min(k - 1, 15)
    if v == "k":
        return min(k, 15)
    return int(v)


def entries():
    """Every sweep entry as (option name, Opt), in table order."""
    return [(name, o) for name, opts in SWEEP.items() for o in opts]


def describe(name: str, o: Opt) -> str:
    s = f"{name}={o.value}"
    if o.with_:
        s += " with " + ",".join(f"{a}={b}" for a, b in o.with_.items())
    if o.env:
        s += " env " + ",".join(f"{a}={b}" for a, b in o.env.items())
    return s + ("" if o.form == "single" else f" [{o.form}]")
