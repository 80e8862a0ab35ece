"""The result file of a run of cfg4's size read two ways: the host reader (extract.parse_result + ResultArrays.from_result,
the parent's code) and the device reader (slice.read_arrays(reader="device"): asgart_result_scan, asgart_result_parse).

    python tools/read_bench.py [out.json] [--quick]

The synthetic results of tools/export_bench.py -- 140 113 duplications (cfg4 after the reduction) and 689 093 (before it)
in 71 521 families, with identities, as the pretty JSON the device writer gives.  Per case, both ways in this process on this
box, from the file's bytes in memory:
  host_s           read_arrays(reader="host"): median of 5, with the spread (max - min)
  device_s         read_arrays(reader="device"): median of 5 after a warm-up, with the spread
  device           by stage, medians: upload_ms, scan_ms (the four passes and their carries), head_ms (strand and settings
                   parsed on the host, the name table), parse_ms (tokens, offsets, records), copy_ms (the arrays back),
                   fixup_ms (hard names and identities, the ids), and the hard counts
  scan_gb_s        the bytes of the file over scan_ms + parse_ms
  identical        every array of the two results is equal (identity by its bits)
  device_wins      the device median is below the host median by more than both spreads together
Prints one JSON line with the commit; the device reader is the tools' default if device_wins holds at both sizes.
--quick: one small case (a rehearsal)."""
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
from export_bench import with_identities  # noqa: E402
from slice_bench import make_arrays  # noqa: E402

STAGES = ("upload_ms", "scan_ms", "head_ms", "parse_ms", "copy_ms", "fixup_ms")


def identical(a: sl.ResultArrays, b: sl.ResultArrays) -> bool:
    return (a.names == b.names and a.strand_name == b.strand_name and a.strand_length == b.strand_length
            and a.settings == b.settings and a.seqs == b.seqs
            and all(np.array_equal(getattr(a, f), getattr(b, f))
                    for f in ("map_name", "map_pos", "map_len", "offs", "sds", "flags", "chr", "chr_pos"))
            and np.array_equal(a.identity.view(np.uint32), b.identity.view(np.uint32)))


def timed(fn, reps):
    out, times = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


def bench_case(data: bytes, reps: int = 5) -> dict:
    want, host = timed(lambda: sl.read_arrays([data], reader="host"), reps)
    sl.read_arrays([data], reader="device")                   # (the first call loads the code object)
    stages = []
    got, device = timed(lambda: sl.read_arrays([data], reader="device", stages=stages), reps)
    dev = {k: round(statistics.median(s[k] for s in stages), 3) for k in STAGES}
    dev["hard_names"], dev["hard_identities"] = stages[-1]["hard_names"], stages[-1]["hard_identities"]
    host_s, device_s = statistics.median(host), statistics.median(device)
    spread = (max(host) - min(host)) + (max(device) - min(device))
    return {"file_bytes": len(data), "host_s": round(host_s, 4), "host_spread_s": round(max(host) - min(host), 4),
            "device_s": round(device_s, 4), "device_spread_s": round(max(device) - min(device), 4), "device": dev,
            "speedup": round(host_s / device_s, 2),
            "scan_gb_s": round(len(data) / ((dev["scan_ms"] + dev["parse_ms"]) * 1e6), 1),
            "identical": identical(got, want), "device_wins": bool(host_s - device_s > spread)}


def main():
    args = sys.argv[1:]
    out_path = next((a for a in args if a.endswith(".json")), None)
    quick = "--quick" in args
    sizes = [(3_000, 1_500)] if quick else [(140_113, 71_521), (689_093, 71_521)]
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    tile, per_block, stage = asgart_amd.result_geometry()
    res = {"commit": commit or None, "geometry": {"tile_bytes": tile, "records_per_block": per_block, "stage_bytes": stage},
           "cases": []}
    for n, n_fam in sizes:
        data = sl.export_arrays_gpu(with_identities(make_arrays(n, n_fam), True), "json")
        case = {"duplications": n, "families": n_fam}
        case.update(bench_case(data, 2 if quick else 5))
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    res["device_is_default"] = all(c["device_wins"] for c in res["cases"])
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(c["identical"] for c in res["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
