"""The filters of asgart-plot on a result of cfg4's size -- 689 093 duplications in 71 521 families, built as
tools/slice_bench.py builds them -- against a synthetic annotation of 100 000 positions, all three feature filters on.

    python tools/plot_bench.py [out.json] [--dups N --families F] [--positions P] [--sample S]

The annotation is built from a seed: 80 000 single-position features as a GFF3 file gives them (fragment + offset) and
2 000 features of ten absolute positions each, lengths 500 .. 50 000, spread over the strand by fragment length.
Timed, for `--min-length 2000 --max-identity 100 --filter-families 10000 --filter-duplicons 1000 --filter-features 5000`:
  per_object_sample_s   plot.apply on the dict form of the first families that hold `--sample` duplications (default 40)
                        against the WHOLE annotation: the statement tests every duplication against every position, the
                        whole result would take hours.  per_object_extrapolated_s scales it by duplications.
  arrays_s              plot.apply_arrays on the whole result: resolving the positions, the upload, the kernels, the copy
                        back, the gather by keys
  sorted / literal      the call and its kernels by HIP events (asgart_plot_timings: whole call, first to last kernel, the
                        joins), warmed up, median of `runs`: the sorted path, and every pair through the literal kernel
The survivors of the sample under both forms, and of the whole result under both paths, are compared.  Prints one JSON line
with the commit.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from asgart_amd import plot  # noqa: E402
from asgart_amd import slice as sl  # noqa: E402
from slice_bench import make_arrays  # noqa: E402


def make_tracks(arr: sl.ResultArrays, n_pos: int, seed: int = 9):
    rng = np.random.default_rng(seed)
    n_multi = n_pos // 50                                    # features of ten positions: a fifth of the positions
    n_single = n_pos - 10 * n_multi
    lens = arr.map_len.astype(np.float64)
    frag = rng.choice(len(lens), size=n_single, p=lens / lens.sum())
    off = (rng.random(n_single) * lens[frag]).astype(np.int64)
    length = rng.integers(500, 50_000, size=n_pos)
    gff = [{"name": f"gene{k}", "positions": [{"chr": arr.names[arr.map_name[frag[k]]], "start": int(off[k]),
                                               "length": int(length[k])}]} for k in range(n_single)]
    start = rng.integers(0, arr.strand_length, size=10 * n_multi)
    custom = [{"name": f"family{k}", "positions": [{"chr": None, "start": int(start[10 * k + j]),
                                                    "length": int(length[n_single + 10 * k + j])} for j in range(10)]}
              for k in range(n_multi)]
    return [gff, custom]


def sample_of(arr: sl.ResultArrays, n_sample: int) -> sl.ResultArrays:
    f = int(np.searchsorted(arr.offs, n_sample, side="left"))
    n = int(arr.offs[f])
    return sl.ResultArrays(arr.strand_name, arr.strand_length, arr.settings, arr.names, arr.map_name, arr.map_pos,
                           arr.map_len, arr.offs[:f + 1], arr.sds[:n], arr.flags[:n], arr.chr[:n], arr.chr_pos[:n],
                           arr.identity[:n])


def timed_calls(arr, ta, options, runs):
    c = plot._c_options(options)
    out = plot.plot_filter(arr.offs, arr.sds, arr.identity, ta, c)        # (the first call loads the code object)
    ms = []
    for _ in range(runs):
        t = []
        plot.plot_filter(arr.offs, arr.sds, arr.identity, ta, c, timings=t)
        ms.append(t)
    return out, {"runs": runs, "call_ms_median": round(statistics.median(m[0] for m in ms), 3),
                 "kernels_ms_median": round(statistics.median(m[1] for m in ms), 3),
                 "joins_ms_median": round(statistics.median(m[2] for m in ms), 3),
                 "joins_ms_min": round(min(m[2] for m in ms), 3)}


def bench(n: int, n_fam: int, n_pos: int, n_sample: int) -> dict:
    arr = make_arrays(n, n_fam)
    tracks = make_tracks(arr, n_pos)
    options = plot.PlotOptions(min_length=2000, min_identity=0.0, max_identity=100.0, filter_families=10_000,
                               filter_duplicons=1000, filter_features=5000)
    sample = sample_of(arr, n_sample)
    result = sample.to_result()
    t0 = time.perf_counter()
    want = plot.apply(result, [list(t) for t in tracks], options)
    per_object_s = time.perf_counter() - t0
    got = plot.apply_arrays(sample, tracks, options)
    sample_same = got[0].to_result() == want[0] and got[1] == want[1]
    plot.apply_arrays(arr, tracks, options)
    t0 = time.perf_counter()
    out, kept = plot.apply_arrays(arr, tracks, options)
    arrays_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ta = plot.resolve_tracks(arr._strand_dict()["map"], tracks)
    resolve_s = time.perf_counter() - t0
    a, sorted_ms = timed_calls(arr, ta, options, 7)
    literal = plot.PlotOptions(**{**options.__dict__, "force_literal": True})
    b, literal_ms = timed_calls(arr, ta, literal, 3)
    paths_same = all((x == y).all() for x, y in zip(a, b))
    return {"duplications": n, "families": n_fam, "positions": int(len(ta.start)), "features": int(len(ta.feat_offsets) - 1),
            "survivors": int(out.n), "families_left": int(len(out.offs) - 1), "features_left": int(sum(len(t) for t in kept)),
            "per_object_sample_duplications": int(sample.n), "per_object_sample_s": round(per_object_s, 3),
            "per_object_extrapolated_s": round(per_object_s * n / max(sample.n, 1), 0),
            "sample_identical": bool(sample_same), "arrays_s": round(arrays_s, 4), "resolve_positions_s": round(resolve_s, 4),
            "sorted": sorted_ms, "literal": literal_ms, "paths_identical": bool(paths_same)}


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default

    n, n_fam = opt("--dups", 689_093), opt("--families", 71_521)
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    res = {"commit": commit or None, "plot": bench(n, n_fam, opt("--positions", 100_000), opt("--sample", 40))}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["plot"]["sample_identical"] and res["plot"]["paths_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
