"""The paralogy groups of a result of cfg4's size -- tools/rosary_bench.py's synthetic result: 689 093 duplications in 71 521
families on 24 fragments -- and two shapes built against the union-find.

    python tools/groups_bench.py [out.json] [--dups N --families F] [--runs R] [--adversarial N]

Timed in one process, `runs` times each (default 5), reported as the median and the spread (max - min):
  host_s        groups.groups_host, the readable statement: a sorted fold and a plain union-find, per object
  scipy_s       the same arrays from numpy and scipy: one lexsort, a running maximum per name (np.maximum.accumulate on ends
                offset by the name, which needs ends + margin below 2^40), scipy.sparse.csgraph.connected_components over the
                loci, bincounts.  Where scipy cannot be imported the entry says so and nothing is timed.
  device        asgart_groups_timings of groups.duplication_groups, warmed up: upload, kernels from the first to the last,
                copy back; and call_s, the whole Python call
Every output array of the three is compared for equality.  Then, for the kernels alone (asgart_groups_timings[1]), checked
against the scipy form (or the host statement without scipy):
  path          N + 1 loci in one path, its N edges in random order
  star_hub_last N leaves on one hub that is the LARGEST locus: whichever leaf hooks the hub first, every other edge meets a
                root that has moved
  star_hub_first the same with the hub the smallest locus: every hook goes under the same root, none is contended
Prints one JSON line with the commit.
"""
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from asgart_amd import groups  # noqa: E402
from rosary_bench import N_FRAGMENTS, make_arrays  # noqa: E402

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    SCIPY = True
except ImportError:
    SCIPY = False

FIELDS = [f.name for f in dataclasses.fields(groups.Groups)]


def groups_scipy(name, start, length, margin, n_names) -> groups.Groups:
    """The arrays of groups_host from numpy and scipy.  Ends + margin must stay below 2^40 and name ids below 2^22: the
    running maximum per name is one np.maximum.accumulate over ends offset by name << 40."""
    name, start, length = name.astype(np.int64), start.astype(np.int64), length.astype(np.int64)
    m = len(name)
    end = start + length
    assert m > 0 and int(end.max()) + margin < 1 << 40 and n_names < 1 << 22
    order = np.lexsort((start, name))
    nm, st, en = name[order], start[order], end[order]
    run = np.maximum.accumulate(en + (nm << 40)) - (nm << 40)
    head = np.ones(m, dtype=bool)
    head[1:] = (nm[1:] != nm[:-1]) | (st[1:] >= run[:-1] + margin)
    first = np.flatnonzero(head)
    last = np.concatenate([first[1:], [m]]) - 1
    locus = np.cumsum(head) - 1
    arm_locus = np.empty(m, dtype=np.int64)
    arm_locus[order] = locus
    n_loci = len(first)
    a, b = arm_locus[0::2], arm_locus[1::2]
    _, label = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n_loci, n_loci)), directed=False)
    _, where = np.unique(label, return_index=True)          # the smallest locus of every label
    rank = np.empty(len(where), dtype=np.int64)
    rank[np.argsort(where, kind="stable")] = np.arange(len(where))
    locus_group = rank[label]
    group = locus_group[a]
    l_length = (run[last] - st[first]).astype(np.uint64)
    g_dups = np.bincount(group, minlength=len(where))
    g_bases = np.zeros(len(where), dtype=np.uint64)
    np.add.at(g_bases, locus_group, l_length)
    return groups.Groups(np.searchsorted(nm[first], np.arange(n_names + 1), side="left").astype(np.int64),
                         nm[first].astype(np.int32), st[first].astype(np.uint64), l_length,
                         (last - first + 1).astype(np.uint32), locus_group.astype(np.uint32),
                         np.bincount(locus_group, minlength=len(where)).astype(np.uint32), g_dups.astype(np.uint32), g_bases,
                         group.astype(np.uint32), np.argsort(group, kind="stable").astype(np.int64),
                         np.concatenate([[0], np.cumsum(g_dups)]).astype(np.int64), arm_locus.astype(np.uint32))


def equal(a: groups.Groups, b: groups.Groups) -> bool:
    return all(getattr(a, f).dtype == getattr(b, f).dtype and np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def figure(values, digits=3):
    return {"median": round(statistics.median(values), digits), "spread": round(max(values) - min(values), digits)}


def timed(fn, runs):
    out, seconds = None, []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        seconds.append(time.perf_counter() - t0)
    return out, figure(seconds, 4)


def timed_device(args, runs):
    out = groups.duplication_groups(*args)   # (the first call loads the code object)
    ms, calls = [], []
    for _ in range(runs):
        t = []
        t0 = time.perf_counter()
        out = groups.duplication_groups(*args, timings=t)
        calls.append(time.perf_counter() - t0)
        ms.append(t)
    return out, {"runs": runs, "upload_ms": figure([m[0] for m in ms]), "kernels_ms": figure([m[1] for m in ms]),
                 "copy_back_ms": figure([m[2] for m in ms]), "call_s": figure(calls, 4)}


def edges_to_arms(edges):
    """Locus x is [100 x, 100 x + 3) on one name; every duplication has an arm in each locus of its edge."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1)
    return np.zeros(len(e), np.int32), (100 * e).astype(np.uint64), np.full(len(e), 3, np.uint64), 0, 1


def adversarial(n, runs):
    rng = np.random.default_rng(10)
    at = rng.permutation(n)
    leaves_last, leaves_first = rng.permutation(n), 1 + rng.permutation(n)
    shapes = {"path": np.column_stack([at, at + 1]),
              "star_hub_last": np.column_stack([np.full(n, n), leaves_last]),
              "star_hub_first": np.column_stack([leaves_first, np.zeros(n, np.int64)])}
    out = {}
    for shape, edges in shapes.items():
        args = edges_to_arms(edges)
        got, ms = timed_device(args, runs)
        want = groups_scipy(*args) if SCIPY else groups.groups_host(*args)
        out[shape] = {"loci": got.n_loci, "groups": got.n_groups, "duplications": n, "kernels_ms": ms["kernels_ms"],
                      "checked_against": "scipy form" if SCIPY else "groups_host", "identical": equal(got, want)}
    return out


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default

    n, n_fam, runs = opt("--dups", 689_093), opt("--families", 71_521), opt("--runs", 5)
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    arr = make_arrays(n, n_fam)
    res = {"commit": commit or None, "groups": {"duplications": n, "families": n_fam, "arms": 2 * n, "fragments": N_FRAGMENTS,
                                                "runs": runs, "margins": []}}
    ok = True
    for margin in (0, 100_000):
        call = (arr.chr.reshape(-1), arr.chr_pos.reshape(-1), np.ascontiguousarray(arr.sds[:, 2:4]).reshape(-1), margin,
                len(arr.names))
        got, device = timed_device(call, runs)
        host, host_s = timed(lambda: groups.groups_host(*call), runs)
        entry = {"margin": margin, "loci": got.n_loci, "groups": got.n_groups, "largest_group_loci": int(got.group_loci.max()),
                 "largest_locus_arms": int(got.locus_members.max()), "duplicated_bases": int(got.locus_length.sum()),
                 "host_s": host_s, "device": device, "device_equals_host": equal(got, host)}
        if SCIPY:
            sp, entry["scipy_s"] = timed(lambda: groups_scipy(*call), runs)
            entry["scipy_equals_host"] = equal(sp, host)
            ok = ok and entry["scipy_equals_host"]
        else:
            entry["scipy_s"] = "not measured: scipy cannot be imported on this machine"
        ok = ok and entry["device_equals_host"]
        res["groups"]["margins"].append(entry)
    res["groups"]["adversarial"] = adversarial(opt("--adversarial", 1_000_000), runs)
    ok = ok and all(v["identical"] for v in res["groups"]["adversarial"].values())
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
