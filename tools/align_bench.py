"""Index.align on a synthetic list of diverged copies, by stage, beside the score kernels on the same list.

    python tools/align_bench.py [out.json] [--pairs N] [--long BP] [--runs R] [--max-distance auto|N] [--banded-only BP]

The list: N regions of 1 .. 20 kb (log-uniform), each against its copy further on in the text with 1.2 % substitutions and
a few short indels (tools/pole_synth.py's "region against its diverged copy", many times over); every other copy is stored
reverse-complemented and aligned with flag 3.  --long BP adds one pair of BP x BP bases as a list of its own: one wave walks
it, whatever its size.

Recorded per list, medians of R runs (default 5) with the smallest and the largest:
  stages_ms        asgart_alignment_timings: upload, forward pass, traceback + compaction, copy back (inclusive = 1, the
                   strings the score compares)
  align_wall_ms    the whole Index.align call
  score_wall_ms    Index.compute_scores_flags on the same list in the same process: the yardstick of the forward pass (the
                   call has no stage timings: its upload and its read-back of one float per pair are in the figure)
  checkpoint_bytes asgart_align_bytes, summed, and the largest
--max-distance auto|N: Index.align(max_distance=) -- the corridor kernels, with the library's bounds or with N for every pair
-- runs beside the full pass on the same list in the same process, and every list gains
  banded           stages_ms and wall_ms of that call, its rounds and cells (asgart_alignment_rounds), its checkpoint bytes
                   for the bounds it ended with, cells_ratio (full cells / banded cells: what the corridor should buy) and
                   forward_ratio, wall_ratio (full median / banded median: what it bought), and whether every entry was
                   bit-equal to the full pass's
--banded-only BP (default 1 000 000 with --max-distance, 0: none) adds one pair of BP x BP bases at 2 % divergence that the
full pass cannot take in a sitting: the corridor call alone is timed (R runs), replayed on the host and its identity
compared with the score's; the full pass's time is ARITHMETIC, labelled so: BP^2 cells at the cells per millisecond the
full forward pass reached on the --long pair in this process.
No time is gated.  Every result is replayed on the host (align.replay) and its identity compared with the score's, bit for
bit.  Prints one JSON line with the commit.
"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import asgart_amd  # noqa: E402
from asgart_amd import align  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP_IDX = np.array([3, 2, 1, 0])


def diverged(rng, a, sub=0.012, indels_per_kb=0.5):
    b = a.copy()
    mut = rng.random(b.shape) < sub
    b[mut] = (b[mut] + rng.integers(1, 4, size=int(mut.sum()))) & 3
    for at in sorted(rng.integers(0, len(b), size=int(len(b) / 1000 * indels_per_kb)).tolist(), reverse=True):
        ln = int(rng.integers(1, 12))
        b = np.delete(b, slice(at, at + ln)) if rng.random() < 0.5 else np.insert(b, at, rng.integers(0, 4, size=ln))
    return b


def make_list(lengths, seed=5):
    """-> (text, sds in inclusive lengths, flags)"""
    rng = np.random.default_rng(seed)
    parts, rows, flags, at = [], [], [], 0
    for k, bp in enumerate(lengths):
        a = rng.integers(0, 4, size=int(bp))
        b = diverged(rng, a)
        flag = 3 if k % 2 else 0
        if flag:
            b = COMP_IDX[b[::-1]]
        gap = rng.integers(0, 4, size=200)
        rows.append((at, at + len(a) + len(gap), len(a) - 1, len(b) - 1))
        flags.append(flag)
        parts += [a, gap, b, gap]
        at += len(a) + len(b) + 2 * len(gap)
    text = np.concatenate([BASES[np.concatenate(parts)], np.frombuffer(b"$", dtype=np.uint8)])
    return text, np.array(rows, dtype=np.uint64), np.array(flags, dtype=np.uint8)


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def stage_spreads(stages):
    return {"upload": spread([s[0] for s in stages]), "forward": spread([s[1] for s in stages]),
            "traceback_compact": spread([s[2] for s in stages]), "copy_back": spread([s[3] for s in stages])}


def same_alignments(x, y):
    return bool(all(np.array_equal(getattr(x, f), getattr(y, f)) for f in
                    ("run_offsets", "run_len", "run_op", "distance", "status")) and
                np.array_equal(x.identity.view(np.uint32), y.identity.view(np.uint32)))


def banded_bytes(sds, got, max_distance):
    """The checkpoint bytes of the bounds the call ended with: the given one, or the first automatic bound that holds the
    pair's distance."""
    if max_distance != "auto":
        return asgart_amd.align_bytes_banded(sds, max_distance, inclusive=True)
    ended = [next(t for t in align.auto_bounds(int(ll) + 1, int(rl) + 1) if t >= d)
             for (ll, rl), d in zip(sds[:, 2:].tolist(), got.distance.tolist())]
    return asgart_amd.align_bytes_banded(sds, np.array(ended, dtype=np.uint32), inclusive=True)


def bench_banded(idx, sds, flags, runs, max_distance):
    """-> (the result, the record) of Index.align(max_distance=) on a list: R timed runs after one that loads the code."""
    rounds = []
    got = idx.align(sds, flags, inclusive=True, max_distance=max_distance, rounds=rounds)
    stages, wall = [], []
    for _ in range(runs):
        t = []
        t0 = time.perf_counter()
        idx.align(sds, flags, inclusive=True, max_distance=max_distance, timings=t)
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(t)
        print(f"align_bench: corridor run of {wall[-1]:.0f} ms", file=sys.stderr, flush=True)   # (a long pair takes a while)
    need = banded_bytes(sds, got, max_distance) if (got.status == 1).all() else np.zeros(1, np.uint64)
    return got, {"max_distance": max_distance, "rounds": rounds[0], "cells": float(rounds[1]),
                 "stages_ms": stage_spreads(stages), "wall_ms": spread(wall),
                 "checkpoint_bytes": {"sum": int(need.sum()), "largest": int(need.max())},
                 "beyond_the_bound": int((got.status == 2).sum())}


def bench_list(name, lengths, runs, max_distance=None):
    text, sds, flags = make_list(lengths)
    need = asgart_amd.align_bytes(sds, inclusive=True)
    with asgart_amd.Index(text, None) as idx:
        full_rounds = []
        got = idx.align(sds, flags, inclusive=True, rounds=full_rounds)   # (the first call loads the code object)
        score = idx.compute_scores_flags(sds, flags)
        stages, wall, score_wall = [], [], []
        for _ in range(runs):
            t = []
            t0 = time.perf_counter()
            idx.align(sds, flags, inclusive=True, timings=t)
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(t)
            t0 = time.perf_counter()
            idx.compute_scores_flags(sds, flags)
            score_wall.append((time.perf_counter() - t0) * 1e3)
        banded = None
        if max_distance is not None:
            narrow, banded = bench_banded(idx, sds, flags, runs, max_distance)
            banded["cells_ratio"] = round(full_rounds[1] / max(banded["cells"], 1.0), 2)
            banded["forward_ratio"] = round(spread([s[1] for s in stages])["median"] /
                                            banded["stages_ms"]["forward"]["median"], 2)
            banded["wall_ratio"] = round(spread(wall)["median"] / banded["wall_ms"]["median"], 2)
            banded["bit_equal_to_full"] = same_alignments(narrow, got) if not banded["beyond_the_bound"] else \
                bool(all(narrow.ops(q) == got.ops(q) and narrow.distance[q] == got.distance[q]
                         for q in np.flatnonzero(narrow.status == 1)))
    replayed = all(align.replay(text, sds[q], int(flags[q]), True, got.ops(q)) == got.distance[q] for q in range(len(sds)))
    fwd, back = spread([s[1] for s in stages]), spread([s[2] for s in stages])
    sc = spread(score_wall)
    return {"list": name, "pairs": len(sds), "cells": float(((sds[:, 2] + 1).astype(np.float64) * (sds[:, 3] + 1)).sum()),
            "longest_arm": int(sds[:, 2:].max()) + 1, "runs": runs,
            "stages_ms": {"upload": spread([s[0] for s in stages]), "forward": fwd, "traceback_compact": back,
                          "copy_back": spread([s[3] for s in stages])},
            "align_wall_ms": spread(wall), "score_wall_ms": sc,
            "forward_over_score": round(fwd["median"] / sc["median"], 3),
            "traceback_over_forward": round(back["median"] / fwd["median"], 3),
            "checkpoint_bytes": {"sum": int(need.sum()), "largest": int(need.max())},
            "cigar_runs": int(len(got.run_len)), "edits": int(got.distance.sum()),
            "replayed": bool(replayed and got.status.all()),
            "identity_bit_equal_to_score": bool(np.array_equal(got.identity.view(np.uint32), score.view(np.uint32))),
            **({} if banded is None else {"banded": banded})}


def bench_banded_only(bp, runs, max_distance, full_cells_per_ms):
    """One pair of bp x bp bases at 2 % divergence (1.2 % substitutions would be the other lists'; here 1.7 % and the same
    short indels), the corridor call alone."""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 4, size=int(bp))
    b = diverged(rng, a, sub=0.017)
    gap = rng.integers(0, 4, size=200)
    text = np.concatenate([BASES[np.concatenate([a, gap, b, gap])], np.frombuffer(b"$", dtype=np.uint8)])
    sds = np.array([(0, len(a) + len(gap), len(a) - 1, len(b) - 1)], dtype=np.uint64)
    flags = np.zeros(1, dtype=np.uint8)
    with asgart_amd.Index(text, None) as idx:
        got, rec = bench_banded(idx, sds, flags, runs, max_distance)
        score = idx.compute_scores_flags(sds, flags)
    ok = bool((got.status == 1).all() and align.replay(text, sds[0], 0, True, got.ops(0)) == got.distance[0])
    cells = float(len(a)) * float(len(b))
    full_bytes = int(asgart_amd.align_bytes(sds, inclusive=True)[0])
    return {"list": f"one pair of {bp} bases, 2 % diverged, corridor only", "pairs": 1, "cells": cells,
            "longest_arm": int(max(len(a), len(b))), "runs": runs, "banded": rec,
            "edits": int(got.distance[0]) if ok else None, "cigar_runs": int(len(got.run_len)),
            "cells_ratio": round(cells / max(rec["cells"], 1.0), 2),
            "full_pass_ARITHMETIC_not_measured": {
                "forward_ms": None if not full_cells_per_ms else round(cells / full_cells_per_ms, 0),
                "from": "cells of this pair / cells per ms of the full forward pass on the --long pair in this process",
                "checkpoint_bytes": full_bytes},
            "replayed": ok,
            "identity_bit_equal_to_score": bool(np.array_equal(got.identity.view(np.uint32), score.view(np.uint32)))}


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default

    pairs, long_bp, runs = opt("--pairs", 512), opt("--long", 50_000), opt("--runs", 5)
    max_distance = args[args.index("--max-distance") + 1] if "--max-distance" in args else None
    if max_distance not in (None, "auto"):
        max_distance = int(max_distance)
    only_bp = opt("--banded-only", 1_000_000 if max_distance is not None else 0)
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    rng = np.random.default_rng(1)
    lengths = np.exp(rng.uniform(np.log(1000), np.log(20_000), size=pairs)).astype(np.int64)
    band, lane_rows, tile = asgart_amd.align_geometry()
    res = {"commit": commit or None, "geometry": {"band_rows": band, "lane_rows": lane_rows, "tile_cols": tile},
           "align": [bench_list("diverged copies, 1-20 kb", lengths, runs, max_distance)] +
                    ([bench_list(f"one pair of {long_bp} bases", [long_bp], runs, max_distance)] if long_bp else [])}
    if max_distance is not None and only_bp:
        rate = None
        if long_bp:
            one = res["align"][-1]
            rate = one["cells"] / one["stages_ms"]["forward"]["median"]
        res["align"].append(bench_banded_only(only_bp, runs, max_distance, rate))
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r["replayed"] and r["identity_bit_equal_to_score"] and
                    r.get("banded", {}).get("bit_equal_to_full", True) for r in res["align"]) else 1


if __name__ == "__main__":
    sys.exit(main())
