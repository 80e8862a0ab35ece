"""The PAF file of a list of alignments written two ways: align.paf_text (the host: one format operation per run) and
align.paf_text_gpu (asgart_paf_records, csrc/paf.hip).

    python tools/paf_bench.py [out.json] [--quick] [--cs short|long]

Synthetic Alignments, no index: rows whose runs alternate between `=` (geometric lengths, mean 60) and an edit (`X`, `I` or
`D`, geometric, mean 1.4), a third of them `-` rows, on a strand of 24 fragments.  Three sizes: 512 rows with 80 536 runs (the
list of profiles/align_synth.json), 8 192 rows with 2^20 runs (multi.PAF_DEVICE_MIN_RUNS: from there on the drivers take the
device writer unasked) and 140 113 rows (cfg4's duplications after the reduction) at about 150 runs each.
Per size, both writers in this process on this box, medians of 5 with the spread max - min:
  host       align.paf_text.  Where the whole list takes long it is timed on a stated sample (its first rows: their runs are
             counted) and scaled by runs, as tools/plot_bench.py scales its host figures; the whole list is then written ONCE
             all the same, for the comparison of the bytes, and that one time is given beside the scaled median.
  device     by stage: names_ms (the arms located and the name table, on the host), upload_ms, kernels_ms, copy_back_ms (the
             library's own figures, asgart_export_timings), call_ms (everything, allocations included), decode_ms (UTF-8 bytes
             -> str, what the drivers return); device_s = call + decode, what a driver pays instead of host_s
  identical  the two texts are equal
  device_wins  the reader's rule for a default: the device median is below the host's by more than both spreads
--cs short|long: both writers add the cs:Z: column (align.paf_text(cs=, text=) against asgart_paf_records_cs).  The bases
come from a random text of TEXT_BYTES (ACGT, 2 % N) that is indexed once; the arms lie anywhere in it, on a strand of 24
fragments of that text, and the runs of a row consume its arms exactly, as the writer demands.  The same three sizes, the
same figures; the index build is not part of any of them.
Prints one JSON line with the commit; --quick: two small sizes (a rehearsal)."""
import io
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
from asgart_amd.prep import Start  # noqa: E402

FRAGMENT = 100_000_000
TEXT_BYTES = 1 << 23                                               # of the random text behind --cs, its `$` included


def make_text(seed: int = 20) -> np.ndarray:
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, TEXT_BYTES, p=[0.245, 0.245, 0.245, 0.245, 0.02])].copy()
    text[-1] = ord("$")
    return text


def make_alignments(rows: int, runs: int, seed: int, n_text: int = 0):
    """-> (offs, sds, flags, strand, aln): `rows` duplications in families of about 2, `runs` runs in all.  n_text: the arms
    lie in a text of that many bytes (before its last one) and the strand's 24 fragments cover it"""
    rng = np.random.default_rng(seed)
    counts = rng.multinomial(runs, np.full(rows, 1.0 / rows))
    run_offsets = np.zeros(rows + 1, np.uint64)
    np.cumsum(counts.astype(np.uint64), out=run_offsets[1:])
    first = np.repeat(run_offsets[:-1].astype(np.int64), counts)
    match = (np.arange(runs) - first) % 2 == 0                      # every row starts with an `=` run
    run_len = np.where(match, rng.geometric(1 / 60, runs), rng.geometric(0.7, runs)).astype(np.uint32)
    run_op = np.where(match, ord("="), np.frombuffer(b"XID", np.uint8)[rng.integers(0, 3, runs)]).astype(np.uint8)
    on_left = np.where(run_op != ord("D"), run_len, 0).astype(np.uint64)
    on_right = np.where(run_op != ord("I"), run_len, 0).astype(np.uint64)
    edits = np.where(match, 0, run_len).astype(np.uint64)
    sums = [np.add.reduceat(np.append(v, 0), np.minimum(run_offsets[:-1], runs).astype(np.int64)) * (counts > 0)
            for v in (on_left, on_right, edits)]
    fragment = n_text // 24 if n_text else FRAGMENT
    strand = asgart_amd.Strand("synthetic", None, [Start(f"chr{i + 1}", i * fragment, fragment) for i in range(24)])
    sds = np.zeros((rows, 4), np.uint64)
    sds[:, 2], sds[:, 3] = sums[0], sums[1]
    if n_text:
        sds[:, 0] = rng.integers(0, n_text - sds[:, 2].astype(np.int64))
        sds[:, 1] = rng.integers(0, n_text - sds[:, 3].astype(np.int64))
    else:
        sds[:, 0] = rng.integers(0, 24 * FRAGMENT - 100_000, rows)
        sds[:, 1] = rng.integers(0, 24 * FRAGMENT - 100_000, rows)
    flags = np.where(rng.random(rows) < 1 / 3, 3, 0).astype(np.uint8)
    cuts = np.sort(rng.choice(np.arange(1, rows), max(rows // 2 - 1, 0), replace=False)) if rows > 2 else np.zeros(0, np.int64)
    offs = np.concatenate([[0], cuts, [rows]]).astype(np.uint64)
    aln = asgart_amd.Alignments(run_offsets, run_len, run_op, sums[2].astype(np.uint32), np.zeros(rows, np.float32),
                                np.ones(rows, np.uint8))
    return offs, sds, flags, strand, aln


def spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "spread": round(max(xs) - min(xs), digits)}


def bench_case(rows: int, runs: int, seed: int, sample_rows: int, reps: int = 5, cs=None, text=None, index=None) -> dict:
    offs, sds, flags, strand, aln = make_alignments(rows, runs, seed, len(text) if cs else 0)
    host_kw = dict(cs=cs, text=text) if cs else {}
    dev_kw = dict(cs=cs, index=index) if cs else {}
    # the host: the whole list, or its first sample_rows rows scaled by runs
    scaled = sample_rows < rows
    k = min(sample_rows, rows)
    part, part_runs = aln.part(0, k), int(aln.run_offsets[k])
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        want = align.paf_text([0, k], sds[:k], flags[:k], strand, part, **host_kw)
        host.append((time.perf_counter() - t0) * runs / part_runs)
    whole_once = None
    if scaled:
        t0 = time.perf_counter()
        want = align.paf_text(offs, sds, flags, strand, aln, **host_kw)
        whole_once = round(time.perf_counter() - t0, 4)
    else:
        want = align.paf_text(offs, sds, flags, strand, aln, **host_kw)   # (with the families of the whole list)
    align._paf_text_device(offs, sds, flags, strand, aln, **dev_kw)  # (the first call loads the code object)
    stages = {s: [] for s in ("names", "upload", "kernels", "copy_back", "call", "decode")}
    device = []
    for _ in range(reps):
        ms = {}
        t0 = time.perf_counter()
        data = align._paf_text_device(offs, sds, flags, strand, aln, 0, io.StringIO(), ms, **dev_kw)
        t1 = time.perf_counter()
        got = str(memoryview(data), "utf-8")
        t2 = time.perf_counter()
        for s, v in zip(stages, (ms["names"], ms["upload"], ms["kernels"], ms["copy"], 1e3 * (t1 - t0), 1e3 * (t2 - t1))):
            stages[s].append(v)
        device.append(t2 - t0)
    h, d = spread(host), spread(device)
    return {"rows": rows, "runs": runs, "minus_rows": int((flags == 3).sum()), "file_bytes": len(data),
            "host_s": h, "host_sample": {"rows": k, "runs": part_runs, "scaled_by_runs": scaled, "whole_list_once_s": whole_once},
            "device_s": d, "device_stages_ms": {s + "_ms": spread(v, 3) for s, v in stages.items()},
            "write_gb_s": round(len(data) / (statistics.median(stages["kernels"]) * 1e6), 2),
            "speedup": round(h["median"] / d["median"], 1), "identical": got == want,
            "device_wins": h["median"] - d["median"] > max(h["spread"], d["spread"])}


def main():
    args = sys.argv[1:]
    cs = args[args.index("--cs") + 1] if "--cs" in args else None
    if cs not in (None, "short", "long"):
        sys.exit("--cs short|long")
    out_path = next((a for a in args if a.endswith(".json")), None)
    sizes = [(64, 5_000, 64), (3_000, 90_000, 500)] if "--quick" in args else \
        [(512, 80_536, 512), (8_192, 1 << 20, 8_192), (140_113, 140_113 * 150, 2_000)]
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    threads, per_block, stage = asgart_amd.paf_geometry()
    res = {"commit": commit or None, "reps": 5,
           "geometry": {"block_threads": threads, "runs_per_block": per_block, "stage_bytes": stage}, "cases": []}
    text = index = None
    if cs:
        res["cs"] = cs
        res["geometry"]["solo_bytes"] = asgart_amd.paf_cs_geometry()[3]
        res["text_bytes"] = TEXT_BYTES
        text = make_text()
        index = asgart_amd.Index(text, None)
    for i, (rows, runs, sample) in enumerate(sizes):
        case = bench_case(rows, runs, 21 + i, sample, cs=cs, text=text, index=index)
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    if index is not None:
        index.close()
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(c["identical"] for c in res["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
