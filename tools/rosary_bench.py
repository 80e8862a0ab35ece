"""The rosary plot of a result of cfg4's size -- 689 093 duplications in 71 521 families (tests/golden/digests.json: the two
passes of cfg4) on 24 fragments of human-like lengths, built from a seed -- with --clustering 0 and 100 000.

    python tools/rosary_bench.py [out.json] [--dups N --families F] [--sample-fragments K]

Timed, per clustering margin:
  per_object_s          rosary.rosary_text on the dict form: the statement walks every duplication of the result for every
                        fragment of the map and draws object by object in float32 scalars.  By default the WHOLE map; with
                        --sample-fragments K the map is cut down to its first K fragments (every duplication is still
                        walked for each of them) and per_object_fragments says so.
  arrays_s              rosary.rosary_arrays on the WHOLE result: the library call, the merge, the bead counts, the float32
                        cumsum and the formatting (arrays_rosary_mode_s: the same with --rosary)
  clusters              asgart_rosary_timings of the library call alone, warmed up, median of `runs`: upload, kernels (the two
                        radix sorts, heads, scan, reduction, offsets), copy back
  scheme_s              rosary.clusters_numpy on the same arrays (the parallel statement on the host)
The two outputs are compared byte for byte on the fragments the per-object statement drew; the library's clusters are
compared with the scheme's.  No feature tracks.  Prints one JSON line with the commit.
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

from asgart_amd import rosary  # noqa: E402
from asgart_amd import slice as sl  # noqa: E402

N_FRAGMENTS = 24


def make_arrays(n: int, n_fam: int, seed: int = 4) -> sl.ResultArrays:
    """Family sizes geometric and scaled to the total (digests.json records the counts of cfg4, not its sizes); 24 fragments
    of 45 .. 250 Mb; 60 % of the duplications have both arms on one fragment; arms of 1 .. 5 kb; 95 % of the arms sit in 200
    hot spots of 200 kb per fragment (duplications pile up: clusters of thousands of arms), the rest anywhere (lone squares
    between beads of every size)."""
    rng = np.random.default_rng(seed)
    sizes = rng.geometric(n_fam / n, size=n_fam).astype(np.int64)
    sizes = np.maximum(1, (sizes * (n / sizes.sum())).astype(np.int64))
    sizes[np.argmax(sizes)] += n - int(sizes.sum())
    offs = np.concatenate([[0], np.cumsum(sizes)])
    lens = rng.integers(45_000_000, 250_000_000, size=N_FRAGMENTS)
    names = [f"chr{k + 1}" for k in range(N_FRAGMENTS)]
    left = rng.choice(N_FRAGMENTS, size=n, p=lens / lens.sum()).astype(np.int32)
    right = np.where(rng.random(n) < 0.6, left, rng.choice(N_FRAGMENTS, size=n, p=lens / lens.sum())).astype(np.int32)
    chr_ = np.column_stack([left, right])
    arm = rng.integers(1000, 5_000, size=(n, 2))
    pos = (rng.random((n, 2)) * (lens[chr_] - 20_000)).astype(np.int64)
    hot = rng.random((n, 2)) < 0.95
    spots = (rng.random((N_FRAGMENTS, 200)) * (lens[:, None] - 1_000_000)).astype(np.int64)
    pos = np.where(hot, spots[chr_, rng.integers(0, 200, size=(n, 2))] + rng.integers(0, 200_000, size=(n, 2)), pos)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    sds = np.column_stack([starts[left] + pos[:, 0].astype(np.uint64), starts[right] + pos[:, 1].astype(np.uint64),
                           arm]).astype(np.uint64)
    settings = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500,
                "trim": None, "skip_masked": False}
    return sl.ResultArrays("cfg4-shaped", int(lens.sum()), settings, names, np.arange(N_FRAGMENTS), starts, lens, offs, sds,
                           rng.integers(0, 4, size=n).astype(np.uint8), chr_, pos.astype(np.uint64),
                           rng.random(n).astype(np.float32) * 100)


def first_fragments(arr: sl.ResultArrays, k: int) -> sl.ResultArrays:
    return sl.ResultArrays(arr.strand_name, arr.strand_length, arr.settings, arr.names, arr.map_name[:k], arr.map_pos[:k],
                           arr.map_len[:k], arr.offs, arr.sds, arr.flags, arr.chr, arr.chr_pos, arr.identity)


def cluster_args(arr: sl.ResultArrays):
    return arr.chr.reshape(-1), arr.chr_pos.reshape(-1), np.ascontiguousarray(arr.sds[:, 2:4]).reshape(-1), arr.flags


def timed_clusters(arr, margin, runs):
    args = cluster_args(arr)
    out = rosary.rosary_clusters(*args, margin, len(arr.names))          # (the first call loads the code object)
    ms = []
    for _ in range(runs):
        t = []
        rosary.rosary_clusters(*args, margin, len(arr.names), timings=t)
        ms.append(t)
    return out, {"runs": runs, "upload_ms_median": round(statistics.median(m[0] for m in ms), 3),
                 "kernels_ms_median": round(statistics.median(m[1] for m in ms), 3),
                 "kernels_ms_min": round(min(m[1] for m in ms), 3),
                 "copy_back_ms_median": round(statistics.median(m[2] for m in ms), 3)}


def bench_margin(arr, result, margin, k_sample):
    tracks = []
    sample = first_fragments(arr, k_sample)
    sample_result = dict(result, strand=sample._strand_dict())
    t0 = time.perf_counter()
    want = rosary.rosary_text(sample_result, tracks, margin, False)
    per_object_s = time.perf_counter() - t0
    same = rosary.rosary_arrays(sample, tracks, margin, False) == want   # (also the call that loads the code object)
    t0 = time.perf_counter()
    text = rosary.rosary_arrays(arr, tracks, margin, False)
    arrays_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    beads = rosary.rosary_arrays(arr, tracks, margin, True)
    arrays_rosary_s = time.perf_counter() - t0
    got, ms = timed_clusters(arr, margin, 7)
    t0 = time.perf_counter()
    scheme = rosary.clusters_numpy(*cluster_args(arr), margin, len(arr.names))
    scheme_s = time.perf_counter() - t0
    return {"clustering": margin, "clusters_found": int(len(got[1])), "largest_cluster_arms": int(got[4].max()),
            "clusters_of_both_kinds": int(((got[3] & 4) != 0).sum()),
            "per_object_fragments": f"{k_sample} of {N_FRAGMENTS} " + ("(the whole)" if k_sample == N_FRAGMENTS else "(a sample)"),
            "per_object_s": round(per_object_s, 2), "identical": bool(same), "arrays_s": round(arrays_s, 3),
            "arrays_rosary_mode_s": round(arrays_rosary_s, 3), "svg_bytes": len(text.encode("utf-8")),
            "svg_bytes_rosary_mode": len(beads.encode("utf-8")), "beads": text.count("<circle"),
            "beads_rosary_mode": beads.count("<circle"), "clusters": ms, "scheme_s": round(scheme_s, 4),
            "library_equals_scheme": bool(all((a == b).all() for a, b in zip(got, scheme)))}


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default

    n, n_fam = opt("--dups", 689_093), opt("--families", 71_521)
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    arr = make_arrays(n, n_fam)
    t0 = time.perf_counter()
    result = arr.to_result()
    to_result_s = time.perf_counter() - t0
    res = {"commit": commit or None,
           "rosary": {"duplications": n, "families": n_fam, "arms": 2 * n, "fragments": N_FRAGMENTS,
                      "to_result_s": round(to_result_s, 2),
                      "margins": [bench_margin(arr, result, m, min(opt("--sample-fragments", N_FRAGMENTS), N_FRAGMENTS))
                                  for m in (0, 100_000)]}}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    ok = all(m["identical"] and m["library_equals_scheme"] for m in res["rosary"]["margins"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
