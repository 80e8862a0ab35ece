"""Chaining, host against device, on four shapes.

    python tools/chain_bench.py [out.json] [--runs R] [--sample ANCHORS] [--no-device]

  (a) cfg4       tools/rosary_bench.py's synthetic result of cfg4's size (689 093 duplications, 24 fragments, arms placed
                 without regard to each other), max_gap and lookback at their defaults
  (b) fragmented 10 000 duplications of 100 kb, each cut into 64 anchors: gaps drawn from 100 .. 5 000 bases and capped
                 below the score the chain has reached (a piece behind a gap longer than everything in front of it is a
                 new duplication by the rule), the right gap shorter than the left by an indel below the gap; 24
                 fragments, a third of the duplications reversed, the rows shuffled.  Exactly 10 000 chains of 64 are
                 expected and asserted, in every form
  (c) serial     one group of 10^5 anchors, each overlapping the one in front: no segment boundary, one wave walks them
                 all; the time per anchor is reported
  (d) lookback   shape (b) at H = 64 and at H = 1024

Timed in one process, `runs` times each (default 5), reported as the median and the spread (max - min):
  host     chain.chain_host.  Where the whole shape is too slow for it -- (a), (b) and (d) -- it is timed on a SAMPLE of whole
           groups (the first groups in key order that hold `--sample` anchors, default 20 000; 5 000 at H = 1024) and the
           figure is scaled by anchors: host_s_scaled = host_s_sample * anchors / sample anchors.  (c) is one group and is
           timed whole.  Every entry says which
  device   asgart_chains_timings of chain.chain_duplications on the WHOLE shape, warmed up: upload, kernels, copy back; and
           call_s, the whole Python call
Every array of the two forms is compared for equality: on the sample (the device form run on the sample too), and for (b)
and (c) on the whole shape as well, with chain_host run once, untimed.  device_wins is the standing rule: the device's
call_s median below the host's (scaled) median by more than both spreads.  Prints one JSON line with the commit.
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

from asgart_amd import chain  # noqa: E402

FIELDS = [f.name for f in dataclasses.fields(chain.Chains)]
N_FRAGMENTS = 24


def equal(a: chain.Chains, b: chain.Chains) -> bool:
    return all(getattr(a, f).dtype == getattr(b, f).dtype and np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def figure(values, digits=4):
    return {"median": round(statistics.median(values), digits), "spread": round(max(values) - min(values), digits)}


def timed(fn, runs):
    out, seconds = None, []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        seconds.append(time.perf_counter() - t0)
    return out, figure(seconds)


def timed_device(args, runs):
    counts = {}
    out = chain.chain_duplications(*args, counts=counts)   # (the first call loads the code object)
    ms, calls = [], []
    for _ in range(runs):
        t = []
        t0 = time.perf_counter()
        out = chain.chain_duplications(*args, timings=t)
        calls.append(time.perf_counter() - t0)
        ms.append(t)
    return out, counts, {"runs": runs, "upload_ms": figure([m[0] for m in ms], 3), "kernels_ms": figure([m[1] for m in ms], 3),
                         "copy_back_ms": figure([m[2] for m in ms], 3), "call_s": figure(calls)}


def fragmented(n_dups=10_000, pieces=64, seed=7):
    """Shape (b) -> (chr, chr_pos, length, flags).  Duplication d lies in a slot of 600 kb of its own on either side, so
    that two duplications of one group are further apart than any max_gap used here."""
    rng = np.random.default_rng(seed)
    piece = 100_000 // pieces
    ll = piece + rng.integers(-200, 201, size=(n_dups, pieces))
    gap_l = np.zeros((n_dups, pieces), np.int64)
    score = ll[:, 0].copy()
    for k in range(1, pieces):
        gap_l[:, k] = np.minimum(rng.integers(100, 5001, n_dups), score - 1)
        score += ll[:, k] - gap_l[:, k]
    assert (gap_l[:, 1:] >= 100).all()
    gap_r = gap_l - (rng.random((n_dups, pieces)) * gap_l).astype(np.int64)     # the indel is below the gap
    gap_r[:, 1:] = np.maximum(gap_r[:, 1:], 1)
    off_l = np.cumsum(gap_l + np.roll(ll, 1, axis=1) * (np.arange(pieces) > 0), axis=1)
    off_r = np.cumsum(gap_r + np.roll(ll, 1, axis=1) * (np.arange(pieces) > 0), axis=1)
    span_r = off_r[:, -1] + ll[:, -1]
    reversed_ = np.arange(n_dups) % 3 == 0
    d = np.arange(n_dups)
    e = rng.permutation(n_dups)
    pl = (d // N_FRAGMENTS * 600_000)[:, None] + off_l
    pr = (e // N_FRAGMENTS * 600_000)[:, None] + np.where(reversed_[:, None], span_r[:, None] - off_r - ll, off_r)
    chr_ = np.stack([np.broadcast_to((d % N_FRAGMENTS)[:, None], pl.shape), np.broadcast_to((e % N_FRAGMENTS)[:, None], pl.shape)],
                    axis=-1)
    pos = np.stack([pl, pr], axis=-1)
    length = np.stack([ll, ll], axis=-1)
    flags = np.broadcast_to(np.where(reversed_, 3, 0)[:, None], pl.shape)
    shuffle = rng.permutation(n_dups * pieces)
    return (chr_.reshape(-1, 2)[shuffle].reshape(-1).astype(np.int32), pos.reshape(-1, 2)[shuffle].reshape(-1).astype(np.uint64),
            length.reshape(-1, 2)[shuffle].reshape(-1).astype(np.uint64), flags.reshape(-1)[shuffle].astype(np.uint8))


def serial(n=100_000):
    k = np.arange(n)
    pos = np.column_stack([10 * k, 10 * k]).reshape(-1).astype(np.uint64)
    return np.zeros(2 * n, np.int32), pos, np.full(2 * n, 1000, np.uint64), np.zeros(n, np.uint8)


def sample_of(anchors, target):
    """The anchors of the first whole groups, in key order, that hold `target` anchors."""
    chr_, pos, length, flags = anchors
    key = (chr_[0::2].astype(np.int64) << 34) | (chr_[1::2].astype(np.int64) << 2) | flags
    keys, sizes = np.unique(key, return_counts=True)
    take = int(np.searchsorted(np.cumsum(sizes), target, side="left")) + 1
    q = np.flatnonzero(key <= keys[min(take, len(keys)) - 1])
    arms = (2 * q[:, None] + np.arange(2)).reshape(-1)
    return (chr_[arms], pos[arms], length[arms], flags[q]), min(take, len(keys)), len(keys)


def measure(name, anchors, n_names, max_gap, lookback, runs, sample, device, whole_check):
    n = len(anchors[3])
    tail = (n_names, max_gap, lookback)
    entry = {"shape": name, "anchors": n, "max_gap": max_gap, "lookback": lookback, "runs": runs}
    if sample and sample < n:
        part, taken, groups = sample_of(anchors, sample)
        m = len(part[3])
        host, host_s = timed(lambda: chain.chain_host(*part, *tail), runs)
        scale = n / m
        entry.update(host="a sample of whole groups, scaled by anchors", host_sample_groups=f"{taken} of {groups}",
                     host_sample_anchors=m, host_s_sample=host_s,
                     host_s_scaled={k: round(v * scale, 3) for k, v in host_s.items()})
        host_figure = entry["host_s_scaled"]
    else:
        part = anchors
        host, host_s = timed(lambda: chain.chain_host(*anchors, *tail), runs)
        entry.update(host="the whole shape", host_s=host_s)
        host_figure = host_s
    entry["host_chains_of_what_it_ran"] = host.n_chains
    ok = True
    if device:
        got, counts, dev = timed_device(anchors + tail, runs)
        entry.update(chains=got.n_chains, links=got.n_links, segments=counts["n_segments"],
                     longest_chain=int(np.diff(got.chain_offsets).max()), device=dev,
                     kernels_us_per_anchor=round(1000 * dev["kernels_ms"]["median"] / n, 4))
        on_part = got if part is anchors else chain.chain_duplications(*part, *tail)
        entry["device_equals_host_on_what_host_ran"] = equal(on_part, host)
        ok = entry["device_equals_host_on_what_host_ran"]
        if whole_check and part is not anchors:
            t0 = time.perf_counter()
            whole = chain.chain_host(*anchors, *tail)
            entry.update(host_whole_once_s=round(time.perf_counter() - t0, 1), host_whole_chains=whole.n_chains,
                         device_equals_host_on_the_whole=equal(got, whole))
            ok = ok and entry["device_equals_host_on_the_whole"]
        entry["device_wins"] = bool(host_figure["median"] - dev["call_s"]["median"] >
                                    max(host_figure["spread"], dev["call_s"]["spread"]))
    return entry, ok


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default

    runs, sample, device = opt("--runs", 5), opt("--sample", 20_000), "--no-device" not in args
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    from rosary_bench import make_arrays

    arr = make_arrays(opt("--dups", 689_093), opt("--families", 71_521))
    cfg4 = (arr.chr.reshape(-1), arr.chr_pos.reshape(-1), np.ascontiguousarray(arr.sds[:, 2:4]).reshape(-1), arr.flags)
    frag = fragmented(opt("--fragmented", 10_000))
    res = {"commit": commit or None, "shapes": []}
    ok = True
    plan = [("a: cfg4", cfg4, len(arr.names), chain.MAX_GAP, chain.LOOKBACK, sample, False),
            ("b: fragmented", frag, N_FRAGMENTS, chain.MAX_GAP, 64, sample, True),
            ("c: serial", serial(opt("--serial", 100_000)), 1, chain.MAX_GAP, 64, 0, False),
            ("d: fragmented, H = 1024", frag, N_FRAGMENTS, chain.MAX_GAP, 1024, sample // 4, False)]
    for name, anchors, n_names, max_gap, lookback, part, whole in plan:
        entry, good = measure(name, anchors, n_names, max_gap, lookback, runs, part, device, whole)
        if name[0] in "bd" and device:
            sizes = np.diff(chain.chain_duplications(*anchors, n_names, max_gap, lookback).chain_offsets)
            entry["chains_of_64"] = int((sizes == 64).sum())
            assert entry["chains"] == len(anchors[3]) // 64 == entry["chains_of_64"], entry
            assert entry.get("host_whole_chains", entry["chains"]) == entry["chains"], entry
        if name[0] in "bd":
            assert entry["host_chains_of_what_it_ran"] * 64 == entry.get("host_sample_anchors", entry["anchors"]), entry
        ok = ok and good
        res["shapes"].append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
    if device:
        res["device_wins_everywhere"] = all(e["device_wins"] for e in res["shapes"])
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
