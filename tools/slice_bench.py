"""The slice of a result of cfg4's size -- 689 093 duplications in 71 521 families (tests/golden/digests.json: the two
passes of cfg4) -- three ways, and a small scored run with and without a filter that drops about half.

    python tools/slice_bench.py [out.json] [--dups N --families F] [--no-run]

The arrays are built from a seed: family sizes geometric (digests.json records the counts of cfg4, not its sizes) and
scaled to the total, 25 fragments of chromosome-like lengths plus 400 small scaffolds, arms mostly on the same fragment.
Timed, for `--collapse --no-inter-relaxed --min-length L -M 500 --keep-fragments ...` (every stage of the slice at work):
  per_object_s     slice.apply on the dict form (the readable statement; building the dict is not counted)
  arrays_s         slice.apply_arrays: the host tables, the upload, the kernels, the copy back, the gather by keys
  kernels_ms       the kernels alone by HIP events (asgart_slice_timings), warmed up, median of 11
and the survivors of the two forms are compared.  The scored run: multi.search_duplications in process with
--compute-score, unsliced and with --slice-min-length at the median arm length.  Prints one JSON line with the commit.
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
from asgart_amd import multi, synth  # noqa: E402
from asgart_amd import slice as sl  # noqa: E402


def make_arrays(n: int, n_fam: int, seed: int = 4) -> sl.ResultArrays:
    rng = np.random.default_rng(seed)
    sizes = rng.geometric(n_fam / n, size=n_fam).astype(np.int64)
    sizes = np.maximum(1, (sizes * (n / sizes.sum())).astype(np.int64))
    sizes[np.argmax(sizes)] += n - int(sizes.sum())
    offs = np.concatenate([[0], np.cumsum(sizes)])
    lens = np.concatenate([rng.integers(40_000_000, 250_000_000, size=25), rng.integers(1_000, 200_000, size=400)])
    names = [f"chr{k + 1}" for k in range(25)] + [f"scaffold_{k}" for k in range(400)] + ["unknown"]
    weights = np.concatenate([lens / lens.sum(), [1e-4]])
    left = rng.choice(len(names), size=n, p=weights / weights.sum()).astype(np.int32)
    right = np.where(rng.random(n) < 0.6, left, rng.choice(len(names), size=n, p=weights / weights.sum())).astype(np.int32)
    arm = rng.integers(1000, 20_000, size=(n, 2))
    pos = (rng.random((n, 2)) * np.concatenate([lens, [1 << 30]])[np.column_stack([left, right])]).astype(np.uint64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1], [0]]).astype(np.uint64)
    sds = np.column_stack([starts[left] + pos[:, 0], starts[right] + pos[:, 1], arm]).astype(np.uint64)
    settings = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500,
                "trim": None, "skip_masked": False}
    return sl.ResultArrays("cfg4-shaped", int(lens.sum()), settings, names, np.arange(425), starts[:-1], lens, offs, sds,
                           rng.integers(0, 4, size=n).astype(np.uint8), np.column_stack([left, right]), pos,
                           rng.random(n).astype(np.float32) * 100)


def bench_slice(n: int, n_fam: int) -> dict:
    arr = make_arrays(n, n_fam)
    opts = sl.SliceOptions(collapse=True, no_inter_relaxed=True, min_length=int(np.median(arr.sds[:, 2:].min(axis=1))),
                           max_family_members=500, keep_fragments=[sl.COLLAPSED_NAME] + [f"chr{k}" for k in range(1, 20)])
    t0 = time.perf_counter()
    result = arr.to_result()
    to_result_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = sl.apply(result, opts)
    per_object_s = time.perf_counter() - t0
    sl.apply_arrays(arr, opts)                               # (the first call loads the code object)
    t0 = time.perf_counter()
    got = sl.apply_arrays(arr, opts)
    arrays_s = time.perf_counter() - t0
    sp = sl.plan(arr, opts)
    ms = []
    for _ in range(11):
        t = []
        sl.slice_families(arr.offs, arr.sds, arr.flags, arr.chr, arr.chr_pos, sp, timings=t)
        ms.append(t)
    same = got.to_result() == want
    return {"duplications": n, "families": n_fam, "survivors": int(got.n), "families_left": int(len(got.offs) - 1),
            "to_result_s": round(to_result_s, 3), "per_object_s": round(per_object_s, 3), "arrays_s": round(arrays_s, 4),
            "call_ms_median": round(statistics.median(m[0] for m in ms), 3),
            "kernels_ms_median": round(statistics.median(m[1] for m in ms), 4),
            "kernels_ms_min": round(min(m[1] for m in ms), 4), "identical": bool(same)}


def bench_run(tmp: str) -> dict:
    recs = synth.make_genome([400_000, 300_000, 300_000], seed=11, sd_per_mb=60, sd_len=(1000, 8000), alu_frac=0.04,
                             l1_frac=0.0, sat_per_record=0)
    path = os.path.join(tmp, "slice_bench.fa")
    with open(path, "w") as fh:
        for name, seq in recs:
            fh.write(f">{name}\n{np.asarray(seq, dtype=np.uint8).tobytes().decode('ascii')}\n")
    st = asgart_amd.RunSettings.from_cli(reverse=True, complement=True)
    out = {}
    multi.search_duplications([path], st, None, 0, compute_score=True)          # warm-up
    t0 = time.perf_counter()
    text, _ = multi.search_duplications([path], st, None, 0, compute_score=True)
    out["unsliced_s"] = round(time.perf_counter() - t0, 3)
    sds = [sd for fam in json.loads(text)["families"] for sd in fam]
    cut = int(np.median([min(sd["left_length"], sd["right_length"]) for sd in sds])) if sds else 0
    t0 = time.perf_counter()
    text, _ = multi.search_duplications([path], st, None, 0, compute_score=True,
                                        slice_options=sl.SliceOptions(min_length=cut))
    out["sliced_s"] = round(time.perf_counter() - t0, 3)
    left = sum(len(fam) for fam in json.loads(text)["families"])
    out.update(duplications=len(sds), survivors=left, min_length=cut)
    return out


def main():
    args = sys.argv[1:]
    n, n_fam = 689_093, 71_521
    if "--dups" in args:
        n = int(args[args.index("--dups") + 1])
        n_fam = int(args[args.index("--families") + 1])
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    res = {"commit": commit or None, "slice": bench_slice(n, n_fam)}
    if "--no-run" not in args:
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            res["scored_run"] = bench_run(tmp)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["slice"]["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
