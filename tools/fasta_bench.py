"""The input step of a run, FASTA file path -> a ready index with chunks and map, the old way against the new one:

    (a) host     prep.read_records -> prep.prepare_records -> Index(text)      (Python line loop, numpy, text uploaded)
    (b) device   prep.read_fasta_gpu                                           (asgart_fasta_read + asgart_fasta_index)

on a synth.config_genome input written as 60-column FASTA (and, with `oneline`, as one line per record: the shape
profiles/orientations_cfg*.json were measured on).

    python tools/fasta_bench.py [cfg3] [60|oneline] [out.json] [runs]

One warm-up of each way, then `runs` (default 5) of each, alternating; median, minimum and maximum per way.  Inside
(b): the library's own split of asgart_fasta_read (host copies into the pinned pieces, host -> device copies and kernels
by HIP events on its streams), the index build as the rest, the kernel stage as GB/s of file bytes, and beside it a
device-to-device copy of as many bytes timed in the same process (the kernels move about four times that copy's one-way
bytes).  The chunks and the map of the two ways are compared.  Prints one JSON line and writes it to out.json (default
profiles/fasta_reader_<cfg>[_oneline].json).
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import asgart_amd  # noqa: E402
from asgart_amd import prep, synth  # noqa: E402

CONFIGS = {"cfg4": (4, 1.0), "cfg3": (3, 1.0), "cfg2": (2, 1.0), "tiny": (2, 0.05)}


def write_fasta(path, recs, cols):
    with open(path, "wb") as fh:
        for name, seq in recs:
            seq = np.asarray(seq, dtype=np.uint8)
            fh.write(b">" + name.encode() + b"\n")
            if cols is None:
                fh.write(seq.tobytes() + b"\n")
                continue
            full = len(seq) // cols * cols
            lines = np.empty((full // cols, cols + 1), dtype=np.uint8)
            lines[:, :cols] = seq[:full].reshape(-1, cols)
            lines[:, cols] = 10
            fh.write(lines.tobytes())
            if full < len(seq):
                fh.write(seq[full:].tobytes() + b"\n")


def host_way(path):
    records = list(prep.read_records(path))
    pr = prep.prepare_records(records, False)
    idx = asgart_amd.Index(pr.data, None, 0)
    return pr, idx


def device_way(path):
    pr, idx, _ = prep.read_fasta_gpu([path], False, 0)
    return pr, idx


def d2d_copy_gbps(n_bytes):
    import torch

    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return n_bytes / best / 1e6


def spread(xs):
    return {"median_s": round(statistics.median(xs), 4), "min_s": round(min(xs), 4), "max_s": round(max(xs), 4),
            "runs_s": [round(x, 4) for x in xs]}


def main():
    import torch

    torch.cuda.init()   # (before the library loads the HIP runtime: the device-to-device copy at the end is torch's)
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
    shape = sys.argv[2] if len(sys.argv) > 2 else "60"
    cols = None if shape == "oneline" else int(shape)
    default = os.path.join(ROOT, "profiles", f"fasta_reader_{name}{'_oneline' if cols is None else ''}.json")
    out_path = sys.argv[3] if len(sys.argv) > 3 else default
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    cfg, scale = CONFIGS[name]
    recs = synth.config_genome(cfg, scale)
    res = {"workload": name, "columns": cols, "bases": int(sum(len(s) for _, s in recs)), "records": len(recs)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, f"{name}.fa")
        write_fasta(path, recs, cols)
        del recs
        res["file_bytes"] = os.path.getsize(path)
        t = {"host": [], "device": []}
        inside = []
        same = True
        for rnd in range(runs + 1):       # round 0 warms both ways up (code objects, allocator pools, the page cache)
            for way, fn in (("host", host_way), ("device", device_way)):
                t0 = time.perf_counter()
                pr, idx = fn(path)
                dt = time.perf_counter() - t0
                sig = (pr.chunks, [(s.name, s.position, s.length) for s in pr.map], idx.n)
                idx.close()
                if way == "host":
                    host_sig = sig
                else:
                    same = same and sig == host_sig
                    if rnd:
                        inside.append(dict(pr.timings, wall=dt * 1e3))
                if rnd:
                    t[way].append(dt)
                del pr, idx
        res["host"] = spread(t["host"])
        res["device"] = spread(t["device"])
        res["identical"] = same
        res["speedup_of_medians"] = round(res["host"]["median_s"] / res["device"]["median_s"], 2)
        res["device_below_host_by_more_than_host_spread"] = bool(
            res["host"]["median_s"] - res["device"]["median_s"] > res["host"]["max_s"] - res["host"]["min_s"])
        med = {k: statistics.median(x[k] for x in inside) for k in inside[0]}
        res["inside_device_ms"] = {
            "read_call": round(med["total"], 2), "host_copies_into_pinned": round(med["stage"], 2),
            "h2d_copies": round(med["h2d"], 2), "kernels": round(med["kernels"], 2),
            "index_and_python": round(med["wall"] - med["total"], 2)}
        res["kernels_gb_per_s_of_file_bytes"] = round(res["file_bytes"] / med["kernels"] / 1e6, 1)
        res["h2d_gb_per_s"] = round(res["file_bytes"] / med["h2d"] / 1e6, 1)
        res["d2d_copy_gb_per_s_same_bytes"] = round(d2d_copy_gbps(res["file_bytes"]), 1)
        t0 = time.perf_counter()
        with open(path, "rb") as fh:
            while fh.read(1 << 26):
                pass
        res["page_cache_read_s"] = round(time.perf_counter() - t0, 4)
    line = json.dumps(res)
    print(line, flush=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
