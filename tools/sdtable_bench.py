"""The duplication table of a list of alignments made two ways: on the host (align.stats_host, then align.sd_table_text) and
on the device (Index.alignment_stats -- asgart_alignment_stats, csrc/alnstats.hip -- then align.sd_table_text_gpu --
asgart_sdtable_records, csrc/sdtable.hip).

    python tools/sdtable_bench.py [out.json] [--quick]

The lists are those of tools/paf_bench.py --cs: the three sizes of profiles/paf_synth.json -- 512 rows with 80 536 runs,
8 192 rows with 2^20 runs, 140 113 rows at about 150 runs each -- over its random text of 8 MiB (ACGT, 2 % N), indexed once;
the index build is not part of any figure.  Per size, both ways in this process on this box, medians of 5 with the spread
max - min:
  host       by stage: stats_s (align.stats_host) and text_s (align.sd_table_text); host_s is their sum.  Where the whole
             list takes long both are timed on a stated sample (its first rows: their runs are counted) and scaled by runs,
             as tools/paf_bench.py scales its host figures; the whole list is then made ONCE all the same, for the
             comparison of the bytes, and that one time is given beside the scaled median
  device     by stage: the counts (upload_ms, kernels_ms, copy_back_ms: the library's own figures; call_ms: everything,
             allocations included) and the writer (names_ms: the arms located, the name table and align.divergence, on the
             host; upload_ms, kernels_ms, copy_back_ms, call_ms, decode_ms); device_s = both calls + decode, what a driver
             pays instead of host_s
  identical  the two texts are equal, and so are the counts
  device_wins  the reader's rule for a default: the device median is below the host's by more than both spreads
The counts kernels alone, on the two shapes that must both keep the device busy: one row whose single `X` run has 10^6
bases, and 10^5 rows of one `1X` run each: kernels_ms of Index.alignment_stats, medians of 5, with the counts compared to
align.stats_host once.
Prints one JSON line with the commit; --quick: two small sizes and smaller kernel shapes (a rehearsal)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import asgart_amd  # noqa: E402
from asgart_amd import align  # noqa: E402
from paf_bench import TEXT_BYTES, make_alignments, make_text, spread  # noqa: E402


def bench_case(rows: int, runs: int, seed: int, sample_rows: int, text, index, reps: int = 5) -> dict:
    offs, sds, flags, strand, aln = make_alignments(rows, runs, seed, len(text))
    scaled = sample_rows < rows
    k = min(sample_rows, rows)
    part, part_runs = aln.part(0, k), int(aln.run_offsets[k])
    stats_s, text_s = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        counts = align.stats_host(text, sds[:k], flags[:k], part)
        t1 = time.perf_counter()
        want = align.sd_table_text([0, k], sds[:k], flags[:k], strand, part, counts)
        t2 = time.perf_counter()
        stats_s.append((t1 - t0) * runs / part_runs)
        text_s.append((t2 - t1) * runs / part_runs)
    whole_once = None
    t0 = time.perf_counter()
    if scaled or len(offs) != 2:   # (with the families of the whole list)
        counts = align.stats_host(text, sds, flags, aln)
        want = align.sd_table_text(offs, sds, flags, strand, aln, counts)
    if scaled:
        whole_once = round(time.perf_counter() - t0, 4)
    align._sd_table_device(offs, sds, flags, strand, aln, index.alignment_stats(sds, flags, aln))   # (loads the code objects)
    names = ("counts_upload", "counts_kernels", "counts_copy_back", "counts_call", "names", "upload", "kernels", "copy_back",
             "call", "decode")
    stages = {s: [] for s in names}
    device = []
    for _ in range(reps):
        cms, ms = [], {}
        t0 = time.perf_counter()
        got_counts = index.alignment_stats(sds, flags, aln, cms)
        t1 = time.perf_counter()
        data = align._sd_table_device(offs, sds, flags, strand, aln, got_counts, 0, io.StringIO(), ms)
        t2 = time.perf_counter()
        got = str(memoryview(data), "utf-8")
        t3 = time.perf_counter()
        for s, v in zip(names, (cms[0], cms[1], cms[2], 1e3 * (t1 - t0), ms["names"], ms["upload"], ms["kernels"], ms["copy"],
                                1e3 * (t2 - t1), 1e3 * (t3 - t2))):
            stages[s].append(v)
        device.append(t3 - t0)
    host = [a + b for a, b in zip(stats_s, text_s)]
    h, d = spread(host), spread(device)
    return {"rows": rows, "runs": runs, "mismatch_bases": int(counts.mismatch.sum()), "file_bytes": len(data),
            "host_s": h, "host_stages_s": {"stats_s": spread(stats_s), "text_s": spread(text_s)},
            "host_sample": {"rows": k, "runs": part_runs, "scaled_by_runs": scaled, "whole_list_once_s": whole_once},
            "device_s": d, "device_stages_ms": {s + "_ms": spread(v, 3) for s, v in stages.items()},
            "speedup": round(h["median"] / d["median"], 1), "identical": got == want and got_counts == counts,
            "device_wins": h["median"] - d["median"] > max(h["spread"], d["spread"])}


def kernel_case(what: str, rows, text, index, reps: int = 5) -> dict:
    """rows: the runs of every duplication; the arms lie one behind the other from the start of the text"""
    n = len(rows)
    run_offsets = np.zeros(n + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=run_offsets[1:])
    run_len = np.array([v for r in rows for v, _ in r], np.uint32)
    run_op = np.array([ord(o) for r in rows for _, o in r], np.uint8)
    aln = asgart_amd.Alignments(run_offsets, run_len, run_op, np.zeros(n, np.uint32), np.zeros(n, np.float32),
                                np.ones(n, np.uint8))
    lens = np.array([sum(v for v, _ in r) for r in rows], np.uint64)          # (`=` and `X` only: both arms)
    left = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    sds = np.column_stack([left, left + np.uint64(len(text) // 2), lens, lens]).astype(np.uint64)
    flags = (np.arange(n) % 4).astype(np.uint8)
    assert int(sds[-1, 1] + sds[-1, 3]) < len(text)
    index.alignment_stats(sds, flags, aln)
    kernels, calls = [], []
    for _ in range(reps):
        ms = []
        t0 = time.perf_counter()
        got = index.alignment_stats(sds, flags, aln, ms)
        calls.append(1e3 * (time.perf_counter() - t0))
        kernels.append(ms[1])
    return {"what": what, "rows": n, "runs": int(run_offsets[-1]), "mismatch_bases": int(got.mismatch.sum()),
            "kernels_ms": spread(kernels, 3), "call_ms": spread(calls, 3),
            "identical": got == align.stats_host(text, sds, flags, aln)}


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    out_path = next((a for a in args if a.endswith(".json")), None)
    sizes = [(64, 5_000, 64), (3_000, 90_000, 500)] if quick else \
        [(512, 80_536, 512), (8_192, 1 << 20, 8_192), (140_113, 140_113 * 150, 2_000)]
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    threads, bases = asgart_amd.alignment_stats_geometry()
    w_threads, w_rows, w_stage = asgart_amd.sdtable_geometry()
    res = {"commit": commit or None, "reps": 5, "text_bytes": TEXT_BYTES,
           "geometry": {"stats_block_threads": threads, "stats_bases_per_block": bases, "writer_block_threads": w_threads,
                        "writer_records_per_block": w_rows, "writer_stage_bytes": w_stage}, "cases": [], "counts_kernels": []}
    text = make_text()
    with asgart_amd.Index(text, None) as index:
        for i, (rows, runs, sample) in enumerate(sizes):
            case = bench_case(rows, runs, 21 + i, sample, text, index)
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        big, many = (10 ** 4, 10 ** 3) if quick else (10 ** 6, 10 ** 5)
        for what, rows in ((f"one row, one X run of {big} bases", [[(1, "="), (big, "X"), (1, "=")]]),
                           (f"{many} rows of one 1X run", [[(1, "X")]] * many)):
            case = kernel_case(what, rows, text, index)
            res["counts_kernels"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(c["identical"] for c in res["cases"] + res["counts_kernels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
