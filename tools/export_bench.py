"""The result file of a run of cfg4's size written two ways: the host array exporters (slice.export_arrays: one format
operation per duplication, the parent's code) and the device writer (slice.export_arrays_gpu: asgart_export_records).

    python tools/export_bench.py [out.json] [--quick]

Results of 140 113 duplications (cfg4 after the reduction; profiles/r06_bench_cfg4_end_to_end.json) and of 689 093 (before
it) in 71 521 families, built from a seed by tools/slice_bench.py's make_arrays, with identities (quotients k / len, as
ComputeScore gives them) and without (zeros); JSON, GFF2 and GFF3.  Per case, both ways in this process on this box:
  host_s           slice.export_arrays, median of 3
  device           by stage, medians of 7 after a warm-up: names_ms (the name table and the head of the file, on the host),
                   upload_ms, kernels_ms, copy_back_ms (the library's own figures, asgart_export_timings), call_ms (the
                   whole library call with its allocations), decode_ms (UTF-8 bytes -> str, what the drivers return)
  device_s         names + call + decode: what the driver pays instead of host_s
  write_gb_s       the bytes of the file over kernels_ms
  identical        the two texts are equal
Prints one JSON line with the commit; --quick: one small case per format (a rehearsal)."""
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
from asgart_amd import slice as sl  # noqa: E402
from slice_bench import make_arrays  # noqa: E402


def with_identities(arr: sl.ResultArrays, scored: bool) -> sl.ResultArrays:
    rng = np.random.default_rng(8)
    if scored:   # 1 - distance / length, as an f32 quotient
        length = arr.sds[:, 2:].max(axis=1).astype(np.float32)
        arr.identity = (np.float32(1) - (rng.random(arr.n) * 0.3 * length).astype(np.int64).astype(np.float32) / length)
        arr.identity = np.ascontiguousarray(arr.identity, dtype=np.float32)
    else:
        arr.identity = np.zeros(arr.n, dtype=np.float32)
    return arr


def median_ms(xs):
    return round(statistics.median(xs), 3)


def bench_case(arr: sl.ResultArrays, fmt: str, host_reps: int = 3, device_reps: int = 7) -> dict:
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = sl.export_arrays(arr, fmt)
        host.append(time.perf_counter() - t0)
    sl._export_arrays_device(arr, fmt)                      # (the first call loads the code object)
    stages = {k: [] for k in ("names", "upload", "kernels", "copy_back", "call", "decode")}
    for _ in range(device_reps):
        t0 = time.perf_counter()
        names, prefix, suffix = sl._export_tables(arr, fmt)
        t1 = time.perf_counter()
        ms = []
        data = asgart_amd.export_records(fmt, arr.offs, arr.sds, arr.flags, arr.identity, arr.chr, arr.chr_pos, names, prefix,
                                         suffix, 0, ms)
        t2 = time.perf_counter()
        got = str(memoryview(data), "utf-8")
        t3 = time.perf_counter()
        for k, v in zip(stages, (1e3 * (t1 - t0), ms[0], ms[1], ms[2], 1e3 * (t2 - t1), 1e3 * (t3 - t2))):
            stages[k].append(v)
    dev = {k + "_ms": median_ms(v) for k, v in stages.items()}
    device_s = (dev["names_ms"] + dev["call_ms"] + dev["decode_ms"]) / 1e3
    return {"format": fmt, "file_bytes": len(data), "host_s": round(statistics.median(host), 4), "device": dev,
            "device_s": round(device_s, 4), "speedup": round(statistics.median(host) / device_s, 2),
            "write_gb_s": round(len(data) / (dev["kernels_ms"] * 1e6), 1), "identical": got == want}


def main():
    args = sys.argv[1:]
    out_path = next((a for a in args if a.endswith(".json")), None)
    sizes = [(3_000, 1_500)] if "--quick" in args else [(140_113, 71_521), (689_093, 71_521)]
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    threads, per_block, stage = asgart_amd.export_geometry()
    res = {"commit": commit or None, "geometry": {"block_threads": threads, "records_per_block": per_block, "stage_bytes": stage},
           "cases": []}
    for n, n_fam in sizes:
        base = make_arrays(n, n_fam)
        for scored in (False, True):
            arr = with_identities(base, scored)
            for fmt in sl.FORMATS:
                case = {"duplications": n, "families": n_fam, "identities": scored}
                case.update(bench_case(arr, fmt, 1 if "--quick" in args else 3, 2 if "--quick" in args else 7))
                res["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(c["identical"] for c in res["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
