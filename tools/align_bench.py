"""Index.align on a synthetic list of diverged copies, by stage, beside the score kernels on the same list.

    python tools/align_bench.py [out.json] [--pairs N] [--long BP] [--runs R]

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


def bench_list(name, lengths, runs):
    text, sds, flags = make_list(lengths)
    need = asgart_amd.align_bytes(sds, inclusive=True)
    with asgart_amd.Index(text, None) as idx:
        got = idx.align(sds, flags, inclusive=True)            # (the first call loads the code object)
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
            "identity_bit_equal_to_score": bool(np.array_equal(got.identity.view(np.uint32), score.view(np.uint32)))}


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default

    pairs, long_bp, runs = opt("--pairs", 512), opt("--long", 50_000), opt("--runs", 5)
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    rng = np.random.default_rng(1)
    lengths = np.exp(rng.uniform(np.log(1000), np.log(20_000), size=pairs)).astype(np.int64)
    band, lane_rows, tile = asgart_amd.align_geometry()
    res = {"commit": commit or None, "geometry": {"band_rows": band, "lane_rows": lane_rows, "tile_cols": tile},
           "align": [bench_list("diverged copies, 1-20 kb", lengths, runs)] +
                    ([bench_list(f"one pair of {long_bp} bases", [long_bp], runs)] if long_bp else [])}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r["replayed"] and r["identity_bit_equal_to_score"] for r in res["align"]) else 1


if __name__ == "__main__":
    sys.exit(main())
