"""Summarise a `rocprofv3 --kernel-trace` run of bench.py: for one step (one launch of probe_count_kernel and what
follows it), each extension-tier kernel's start, end, hardware queue and stream, relative to the first tier launch, and
which tiers shared a queue.

    python tools/tier_queue_trace.py <rocprofv3 output dir> [--step N] [--label TEXT] [-o out.json]

Tier of a kernel: extend_kernel = 1; extend_fast_kernel by workgroup size 64 / 256 / 512 / 1024 = 2 / 4 / 5 / 6;
extend_k8_kernel = 3 (the instantiation with the trailing `true` = the runs over ranges); extend_heavy_kernel = 7 (or
tier 2 / 4 / 6 without the arm-resident kernels: this tool assumes the shipped defaults).  A second launch of a tier's
kernel in one step is an early re-run or a cascade and is listed as such."""
import argparse
import csv
import glob
import json
import os
import sys


def tier_of(name, wg):
    if "extend_k8_kernel" in name:
        return "runs" if name.replace(" ", "").rstrip(")").split(">(")[0].endswith("true") else 3
    if "extend_fast_kernel" in name:
        return {64: 2, 256: 4, 512: 5, 1024: 6}.get(wg)
    if "extend_kernel" in name:
        return 1
    if "extend_heavy_kernel" in name:
        return 7
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--step", type=int, default=-2, help="which step (python index over the probe_count launches)")
    ap.add_argument("--label", default="")
    ap.add_argument("-o", default=None)
    a = ap.parse_args()
    files = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no kernel_trace.csv under {a.dir}")
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "probe_count_kernel" in r["Kernel_Name"] and "true>" not in r["Kernel_Name"]]
    i0 = starts[a.step]
    i1 = starts[a.step + 1] if a.step + 1 < len(starts) and a.step != -1 else len(rows)
    step = rows[i0:i1]
    wg = lambda r: int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 0)
    tier_rows = [(tier_of(r["Kernel_Name"], wg(r)), r) for r in step]
    tier_rows = [(t, r) for t, r in tier_rows if t is not None]
    t0 = min(int(r["Start_Timestamp"]) for _, r in tier_rows)
    seen, out = set(), []
    for t, r in tier_rows:
        kind = "tier" if t == "runs" or t not in seen else "re-run"
        seen.add(t)
        out.append({"tier": t, "kind": kind, "start_ms": round((int(r["Start_Timestamp"]) - t0) * 1e-6, 2),
                    "end_ms": round((int(r["End_Timestamp"]) - t0) * 1e-6, 2), "queue_id": int(r["Queue_Id"]),
                    "stream_id": int(r.get("Stream_Id") or -1), "grid": int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0),
                    "workgroup": wg(r)})
    queues = {}
    for e in out:
        if e["kind"] == "tier":
            queues.setdefault(e["queue_id"], []).append(e["tier"])
    step_ms = (int(step[-1]["End_Timestamp"]) - int(step[0]["Start_Timestamp"])) * 1e-6
    res = {"label": a.label, "step_index": a.step, "kernels_in_step": len(step), "step_span_ms": round(step_ms, 2),
           "extension_span_ms": round(max(e["end_ms"] for e in out), 2),
           "tiers_per_queue": {str(q): ts for q, ts in sorted(queues.items())},
           "shared_queues": {str(q): ts for q, ts in sorted(queues.items()) if len(ts) > 1},
           "tier_kernels": out}
    text = json.dumps(res, indent=1)
    if a.o:
        with open(a.o, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
