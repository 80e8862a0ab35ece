"""What every rank of an N-GPU `--compute-score` costs, measured on ONE GPU: the duplications that survive the steps behind
the search at genome scale are scored once whole (asgart_compute_scores), then, for each N, shard by shard
(asgart_compute_scores_shard: what rank r of N runs), each shard alone on the chip.  The union of the shards must be
bit-equal to the whole call.  The longest duplication is also scored alone: the DP of one duplication is not split, so
that time is the floor under any number of GPUs.

    python tools/score_shard_check.py [N[,N...]=2,4,8] [cfgK=cfg4] [--scale S] [--passes direct|rc|both] [--out FILE]

Writes FILE (default profiles/<cfg>_score_shards.json): per pass the
duplication count, DP cells, the one-call time, per N the shard times and their maximum, and the modelled costs
(asgart_score_costs) of every shard next to them.  No N-GPU run is made by this: one GPU, one shard at a time."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import asgart_amd  # noqa: E402
from asgart_amd import prep, synth  # noqa: E402

args = list(sys.argv[1:])


def _opt(name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


out_path = _opt("--out", None)
scale = float(_opt("--scale", "1.0"))
passes = _opt("--passes", "direct")
ns = [int(x) for x in (args[0] if args else "2,4,8").split(",")]
wl = args[1] if len(args) > 1 else "cfg4"
modes = {"direct": [(False, False)], "rc": [(True, True)], "both": [(False, False), (True, True)]}[passes]
out_path = out_path or os.path.join(ROOT, "profiles", f"{wl}_score_shards.json")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


t0 = time.perf_counter()
recs = synth.config_genome(int(wl[3:]), scale)
pr, idx = prep.prepare_records_gpu(recs, device=0, want_text=False)
bp = sum(l for _, l in pr.chunks)
print(f"{wl} x {scale}: {bp / 1e9:.2f} Gbp in {len(pr.chunks)} chunks, input + index {time.perf_counter() - t0:.1f} s",
      flush=True)
res = {"workload": wl, "scale": scale, "bp": bp,
       "library_build": hashlib.sha256(open(asgart_amd.library_path(), "rb").read()).hexdigest()[:12],
       "method": "one GPU; the duplications that survive FilterNs/ReOrder/ReduceOverlap of a pass (asgart_post_process), "
                 "scored by asgart_compute_scores (one call) and by asgart_compute_scores_shard for every shard r of N, "
                 "each call alone on the chip, wall time with the identities on the host; `longest_ms` = the costliest "
                 "duplication scored alone (the floor: one duplication's DP is not split); `model` = asgart_score_costs "
                 "per shard, in wave-steps",
       "passes": {}}
with idx:
    idx.prepare(20)
    for rev, comp in modes:
        st = asgart_amd.RunSettings.from_cli(reverse=rev, complement=comp)
        (offs, sds), ms_search = timed(lambda: idx.search_duplications_raw(pr.chunks, st))
        (_, kept), ms_post = timed(lambda: idx.post_process(offs, sds))
        cells = (kept[:, 2] + 1).astype(np.float64) * (kept[:, 3] + 1)
        cost = asgart_amd.score_costs(kept).astype(np.float64)
        top = int(np.argmax(cost))
        idx.compute_scores(kept[:8], rev, comp)   # warm-up: workspace, code objects
        whole, ms_whole = timed(lambda: idx.compute_scores(kept, rev, comp))
        _, ms_longest = timed(lambda: idx.compute_scores(kept[top:top + 1], rev, comp))
        name = "rc" if rev else "direct"
        print(f"{name}: search {ms_search:.0f} ms, post-process {ms_post:.0f} ms -> {len(kept)} duplications, "
              f"{cells.sum():.3e} cells, longest arm {int(kept[:, 2:].max())} bp; one call {ms_whole:.0f} ms; the costliest "
              f"duplication ({int(kept[top, 2])} x {int(kept[top, 3])}) alone {ms_longest:.0f} ms", flush=True)
        rec = {"duplications": int(len(kept)), "raw_duplications": int(len(sds)), "cells": float(cells.sum()),
               "longest_arm": int(kept[:, 2:].max()), "one_call_ms": round(ms_whole, 1),
               "longest_lengths": [int(kept[top, 2]), int(kept[top, 3])], "longest_ms": round(ms_longest, 1),
               "longest_cost_frac": round(float(cost[top] / cost.sum()), 4), "model_total": float(cost.sum()), "n": {}}
        for n in ns:
            owner = asgart_amd.score_owners(kept, n)
            union = np.full(len(kept), np.nan, dtype=np.float32)
            shard_ms = []
            for r in range(n):
                part, ms = timed(lambda: idx.compute_scores_shard(kept, rev, comp, shard=r, n_shards=n))
                mine = owner == r
                union[mine] = part[mine]
                shard_ms.append(round(ms, 1))
            same = bool(np.array_equal(union.view(np.uint32), whole.view(np.uint32)))
            model = [float(cost[owner == r].sum()) for r in range(n)]
            rec["n"][str(n)] = {"shard_ms": shard_ms, "max_ms": max(shard_ms),
                                "speedup_vs_one_call": round(ms_whole / max(shard_ms), 2),
                                "model_shard_cost": model, "model_max_over_mean": round(max(model) / (sum(model) / n), 3),
                                "bits_equal_to_one_call": same}
            print(f"  N={n}: per-shard ms {' '.join('%.0f' % t for t in shard_ms)}; max {max(shard_ms):.0f} "
                  f"({ms_whole / max(shard_ms):.2f} x); union bit-equal: {same}", flush=True)
        res["passes"][name] = rec
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", out_path)
