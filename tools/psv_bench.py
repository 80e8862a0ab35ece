"""The variant files of a list of alignments made two ways: on the host (align.variants_host, align.sites_numpy, then
align.psv_table_text and align.psv_vcf_text) and on the device (Index.variants and Variants.sites -- csrc/variants.hip --
then align.psv_table_text_gpu and align.psv_vcf_text_gpu -- csrc/variants_write.hip).

    python tools/psv_bench.py [out.json] [--quick]

The lists are those of tools/sdtable_bench.py: the three sizes of profiles/paf_synth.json -- 512 rows with 80 536 runs,
8 192 rows with 2^20 runs, 140 113 rows at about 150 runs each -- over its random text of 8 MiB (ACGT, 2 % N), indexed once;
the index build is not part of any figure.  Per size, both ways in this process on this box, medians of 5 with the spread
max - min:
  host       by stage: variants_s, sites_s, text_s (both texts); host_s is their sum.  Where the whole list takes long
             all three are timed on a stated sample (its first rows) and scaled by runs, as tools/sdtable_bench.py scales
             its host figures
  device     by stage: the records (upload_ms, kernels_ms, copy_back_ms: the library's own figures; call_ms: everything,
             allocations included), the sites (kernels_ms, call_ms), and each writer (names_ms: the arms located and the name
             table, on the host; upload_ms, kernels_ms, copy_back_ms, call_ms); device_s = all four calls and the two
             decodes, what a driver pays instead of host_s
  identical  the two pairs of texts are equal -- of the whole list, or, where the host is scaled, of the sample, made on
             the device once more for that (compared: "whole list" or "sample")
  device_wins  the reader's rule for a default: the device median is below the host's by more than both spreads
The site stage alone, on the two shapes that must both keep the device busy: 10^6 duplications of one `1X` over ONE pair
of positions (two sites of 10^6 entries each), and one `X` run of 7 * 10^5 bases (about 10^6 entries, every one a site of
its own): kernels_ms of Variants.sites, medians of 5, with the sites compared to align.sites_numpy once.
Prints one JSON line with the commit; --quick: two small sizes and smaller site shapes (a rehearsal)."""
import json
import os
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


def host_texts(text, offs, sds, flags, strand, aln, times=None):
    t0 = time.perf_counter()
    records = align.variants_host(text, sds, flags, aln)
    t1 = time.perf_counter()
    sites = align.sites_numpy(records)
    t2 = time.perf_counter()
    table = align.psv_table_text(offs, sds, flags, strand, records)
    vcf = align.psv_vcf_text(offs, sds, flags, strand, sites, records)
    t3 = time.perf_counter()
    if times is not None:
        times.append((t1 - t0, t2 - t1, t3 - t2))
    return table, vcf, len(records), len(sites)


def device_texts(index, offs, sds, flags, strand, aln, stages=None):
    vms, sms, tms, cms = [], [], {}, {}
    t0 = time.perf_counter()
    with index.variants(sds, flags, aln, vms) as v:
        t1 = time.perf_counter()
        with v.sites(sms) as s:
            t2 = time.perf_counter()
            table = align.psv_table_text_gpu(offs, sds, flags, strand, v, tms)
            t3 = time.perf_counter()
            vcf = align.psv_vcf_text_gpu(offs, sds, flags, strand, s, v, cms)
            t4 = time.perf_counter()
    table, vcf = table.decode("utf-8"), vcf.decode("utf-8")
    t5 = time.perf_counter()
    if stages is not None:
        for name, value in (("records_upload", vms[0]), ("records_kernels", vms[1]), ("records_copy_back", vms[2]),
                            ("records_call", 1e3 * (t1 - t0)), ("sites_kernels", sms[1]), ("sites_call", 1e3 * (t2 - t1)),
                            ("table_upload", tms["upload"]), ("table_kernels", tms["kernels"]), ("table_copy_back", tms["copy"]),
                            ("table_call", 1e3 * (t3 - t2)), ("vcf_upload", cms["upload"]), ("vcf_kernels", cms["kernels"]),
                            ("vcf_copy_back", cms["copy"]), ("vcf_call", 1e3 * (t4 - t3)), ("decode", 1e3 * (t5 - t4))):
            stages.setdefault(name, []).append(value)
    return table, vcf, t5 - t0


def bench_case(rows: int, runs: int, seed: int, sample_rows: int, text, index, reps: int = 5) -> dict:
    offs, sds, flags, strand, aln = make_alignments(rows, runs, seed, len(text))
    scaled = sample_rows < rows
    k = min(sample_rows, rows)
    part, part_runs = aln.part(0, k), int(aln.run_offsets[k])
    part_offs = [0, k] if scaled else offs
    times = []
    for _ in range(reps):
        want = host_texts(text, part_offs, sds[:k], flags[:k], strand, part, times)
    scale = runs / part_runs
    device_texts(index, offs, sds, flags, strand, aln)   # (loads the code objects)
    stages, device = {}, []
    for _ in range(reps):
        table, vcf, seconds = device_texts(index, offs, sds, flags, strand, aln, stages)
        device.append(seconds)
    file_bytes = len(table) + len(vcf)
    n_rows, n_sites = table.count("\n") - 1, sum(not line.startswith("#") for line in vcf.splitlines())
    if scaled:
        table, vcf, _ = device_texts(index, part_offs, sds[:k], flags[:k], strand, part)
    host = [scale * sum(t) for t in times]
    h, d = spread(host), spread(device)
    return {"rows": rows, "runs": runs, "records": n_rows, "sites": n_sites, "file_bytes": file_bytes, "host_s": h,
            "host_stages_s": {name: spread([scale * t[i] for t in times]) for i, name in enumerate(("variants_s", "sites_s", "text_s"))},
            "host_sample": {"rows": k, "runs": part_runs, "scaled_by_runs": scaled, "records": want[2], "sites": want[3]},
            "device_s": d, "device_stages_ms": {name + "_ms": spread(v, 3) for name, v in stages.items()},
            "speedup": round(h["median"] / d["median"], 1), "identical": (table, vcf) == want[:2],
            "compared": "sample" if scaled else "whole list",
            "device_wins": h["median"] - d["median"] > max(h["spread"], d["spread"])}


def sites_case(what: str, sds, rows, text, index, reps: int = 5) -> dict:
    n = len(rows)
    run_offsets = np.zeros(n + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=run_offsets[1:])
    run_len = np.array([v for r in rows for v, _ in r], np.uint32)
    run_op = np.array([ord(o) for r in rows for _, o in r], np.uint8)
    aln = asgart_amd.Alignments(run_offsets, run_len, run_op, np.zeros(n, np.uint32), np.zeros(n, np.float32),
                                np.ones(n, np.uint8))
    flags = np.zeros(n, np.uint8)
    kernels, calls = [], []
    with index.variants(sds, flags, aln) as v:
        with v.sites() as s:
            got = s.arrays()
        for _ in range(reps):
            ms = []
            t0 = time.perf_counter()
            with v.sites(ms) as s:
                calls.append(1e3 * (time.perf_counter() - t0))
                kernels.append(ms[1])
                entries = s.n_entries
        want = align.sites_numpy(v.records())
    return {"what": what, "records": int(run_len.sum()), "entries": entries, "sites": len(got), "kernels_ms": spread(kernels, 3),
            "call_ms": spread(calls, 3), "identical": got == want}


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    out_path = next((a for a in args if a.endswith(".json")), None)
    sizes = [(64, 5_000, 64), (3_000, 90_000, 500)] if quick else \
        [(512, 80_536, 512), (8_192, 1 << 20, 1_024), (140_113, 140_113 * 150, 1_000)]
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    threads, per_block = asgart_amd.variants_geometry()
    w_threads, w_rows, w_stage = asgart_amd.variants_records_geometry()
    res = {"commit": commit or None, "reps": 5, "text_bytes": TEXT_BYTES,
           "geometry": {"records_block_threads": threads, "records_per_block": per_block,
                        "sites_block_threads": asgart_amd.sites_geometry(), "writer_block_threads": w_threads,
                        "writer_rows_per_block": w_rows, "writer_stage_bytes": w_stage}, "cases": [], "sites_kernels": []}
    text = make_text()
    with asgart_amd.Index(text, None) as index:
        for i, (rows, runs, sample) in enumerate(sizes):
            case = bench_case(rows, runs, 21 + i, sample, text, index)
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        many, long_run = (10 ** 4, 7 * 10 ** 3) if quick else (10 ** 6, 7 * 10 ** 5)
        half = len(text) // 2
        left = next(p for p in range(1000, 1100) if text[p] != ord("N"))
        right = next(r for r in range(half, half + 100) if text[r] != text[left] and text[r] != ord("N"))
        one_pair = np.tile(np.array([(left, right, 1, 1)], np.uint64), (many, 1))
        for what, sds, rows in ((f"{many} duplications of 1X over one pair of positions", one_pair, [[(1, "X")]] * many),
                                (f"one X run of {long_run} bases", np.array([(0, half, long_run, long_run)], np.uint64),
                                 [[(long_run, "X")]])):
            case = sites_case(what, sds, rows, text, index)
            res["sites_kernels"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(c["identical"] for c in res["cases"] + res["sites_kernels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
