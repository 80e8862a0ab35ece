"""A masked FASTA of a genome of cfg3's shape (synth.config_genome(3): one record of 249 Mb) and of that record four times
over (996 Mb, four records): the sweep and the writer of asgart_amd.mask, device against numpy, by stage.

    python tools/mask_bench.py [out.json] [--runs R] [--copies K]

The arms come from a synthetic result of cfg4's proportions (tools/rosary_bench.py: 689 093 duplications on 3.1 Gb, arms of
1 .. 5 kb, 95 % of them in 200 hot spots of 200 kb per record), scaled to the strand: 222 duplications per Mb.
Timed in one process, `runs` times each (default 5), reported as the median and the spread (max - min):
  sweep     asgart_mask_timings of mask.mask_intervals, warmed up (upload, kernels, copy back) and call_s, the whole Python
            call; numpy_s: mask.intervals_numpy (its refusals run per object and are timed with it, as the library's are)
  write     asgart_export_timings of mask.write_fasta_gpu, warmed up (upload of the tables, the write kernel, copy back) and
            call_s; kernel_gb_s: (strand bytes read + file bytes written) / the kernel; numpy_s: mask.fasta_text_numpy
  copy      a device-to-device copy (torch, in this process) that reads and writes as many bytes as the write kernel does:
            (strand + file) / 2 bytes copied; gb_s: bytes read + written / its time (HIP events).  The ceiling the write
            kernel is compared with.
  source_upload_s   Source.from_records: the strand to the device, once (the tool's read_fasta_gpu does this from the file)
The device's file is compared with numpy's byte for byte, the intervals array for array.  `device_is_default` states the
rule of the tool's default: the device form's median call is below numpy's by more than both spreads, at every size.
Prints one JSON line with the commit.
"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch  # (before the library loads the HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import asgart_amd  # noqa: E402
from asgart_amd import mask, synth  # noqa: E402

DUPS_PER_MB = 689_093 / 3_100   # cfg4
WIDTH = 60


def figure(values, digits=3):
    return {"median": round(statistics.median(values), digits), "spread": round(max(values) - min(values), digits)}


def timed(fn, runs):
    out, seconds = None, []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        seconds.append(time.perf_counter() - t0)
    return out, figure(seconds, 4)


def make_arms(lens, seed=4):
    """(record, start, length) of 2 n arms, rosary_bench.make_arrays' placement on records of the given lengths."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n = 2 * int(DUPS_PER_MB * lens.sum() / 1e6)
    rec = rng.choice(len(lens), size=n, p=lens / lens.sum()).astype(np.int32)
    arm = rng.integers(1000, 5000, size=n)
    pos = (rng.random(n) * (lens[rec] - 20_000)).astype(np.int64)
    spots = (rng.random((len(lens), 200)) * (lens[:, None] - 1_000_000)).astype(np.int64)
    hot = rng.random(n) < 0.95
    pos = np.where(hot, spots[rec, rng.integers(0, 200, size=n)] + rng.integers(0, 200_000, size=n), pos)
    return rec, pos.astype(np.uint64), arm.astype(np.uint64)


def copy_rate(n_bytes, runs):
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda").fill_(65)
    b = torch.empty_like(a)
    b.copy_(a)
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return {"bytes_copied": n_bytes, "ms": figure(ms), "gb_s": round(2 * n_bytes / statistics.median(ms) / 1e6, 1)}


def bench_size(records, runs):
    lens = [len(r) for r in records]
    headers = [b">chr%d synthetic record %d" % (k + 1, k) for k in range(len(records))]
    rl = np.array(lens, np.uint64)
    rs = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint64)
    arms = make_arms(lens)
    n = int(rl.sum())
    out = {"bases": n, "records": len(records), "arms": len(arms[0]), "width": WIDTH, "runs": runs}

    mask.mask_intervals(*arms, rs, rl)   # (the first call loads the code object)
    ms, calls = [], []
    for _ in range(runs):
        t = []
        t0 = time.perf_counter()
        got = mask.mask_intervals(*arms, rs, rl, timings=t)
        calls.append(time.perf_counter() - t0)
        ms.append(t)
    want, numpy_s = timed(lambda: mask.intervals_numpy(*arms, rs, rl), runs)
    out["sweep"] = {"intervals": got.n, "masked_bases": got.masked_bases, "max_depth": got.max_depth,
                    "upload_ms": figure([m[0] for m in ms]), "kernels_ms": figure([m[1] for m in ms]),
                    "copy_back_ms": figure([m[2] for m in ms]), "call_s": figure(calls, 4), "numpy_s": numpy_s,
                    "device_equals_numpy": bool(np.array_equal(got.intervals, want.intervals) and
                                                (got.masked_bases, got.max_depth) == (want.masked_bases, want.max_depth))}
    iv = got.intervals

    t0 = time.perf_counter()
    src = asgart_amd.Source.from_records(records)
    out["source_upload_s"] = round(time.perf_counter() - t0, 4)
    with src:
        text = mask.write_fasta_gpu(src, rs, rl, headers, iv, WIDTH, 0)
        ms, calls = [], []
        for _ in range(runs):
            t = []
            t0 = time.perf_counter()
            text = mask.write_fasta_gpu(src, rs, rl, headers, iv, WIDTH, 0, timings=t)
            calls.append(time.perf_counter() - t0)
            ms.append(t)
        moved = n + len(text)
        kernel = figure([m[1] for m in ms])
        out["write"] = {"file_bytes": len(text), "upload_ms": figure([m[0] for m in ms]), "kernels_ms": kernel,
                        "copy_back_ms": figure([m[2] for m in ms]), "call_s": figure(calls, 4),
                        "kernel_bytes_read_and_written": moved, "kernel_gb_s": round(moved / kernel["median"] / 1e6, 1)}
        out["copy"] = copy_rate(moved // 2, runs)
    host, out["write"]["numpy_s"] = timed(lambda: mask.fasta_text_numpy(records, headers, iv, WIDTH, 0), runs)
    out["write"]["device_equals_numpy"] = bool(text.tobytes() == host)
    for stage in ("sweep", "write"):
        d, h = out[stage]["call_s"], out[stage]["numpy_s"]
        out[stage]["device_below_numpy_by_more_than_both_spreads"] = bool(h["median"] - d["median"] > d["spread"] + h["spread"])
    return out


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default

    runs, copies = opt("--runs", 5), opt("--copies", 4)
    out_path = next((a for a in args if a.endswith(".json")), None)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    chr1 = np.ascontiguousarray(synth.config_genome(3, 1.0)[0][1], dtype=np.uint8)
    res = {"commit": commit or None, "device": torch.cuda.get_device_name(0), "sizes": []}
    for records in ([chr1], [chr1] * copies):
        res["sizes"].append(bench_size(records, runs))
        print(json.dumps(res["sizes"][-1]), file=sys.stderr, flush=True)
    ok = all(s[stage]["device_equals_numpy"] for s in res["sizes"] for stage in ("sweep", "write"))
    res["device_is_default"] = all(s[stage]["device_below_numpy_by_more_than_both_spreads"] for s in res["sizes"]
                                   for stage in ("sweep", "write"))
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
