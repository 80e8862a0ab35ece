"""One run over several orientations (multi.search_orientations) against one multi.search_duplications run per
orientation -- the way to the same files without it -- on a synth.config_genome input, one GPU, one rank.

    python tools/orientations_bench.py [cfg4] [direct,RC] [out.json] [device|host]

Both ways start from the same FASTA files (written to a temporary directory first) and end with the JSON texts, with and
without --compute-score.  The last argument chooses the drivers' reader (default: theirs, the device reader).  Wall time
of each way, split into prepare (host reader: read_records + prepare_records; device reader: prep.read_fasta_gpu, which
ends with the index built, so `index` is then part of `prepare`), index (Index.__init__: upload, suffix sort), search, post-process and score by timing those calls from outside; `other` is the
rest (JSON writer, gathers).  The texts of the two ways are compared byte for byte.  Prints one JSON line and writes it
to out.json (default profiles/orientations_<cfg>.json).
"""
import json
import os
import sys
import tempfile
import time
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import asgart_amd  # noqa: E402
from asgart_amd import multi, postprocess, prep, synth  # noqa: E402

CONFIGS = {"cfg4": (4, 1.0), "cfg3": (3, 1.0), "cfg2": (2, 1.0), "tiny": (2, 0.05)}
PHASES = {"prepare": [(prep, "read_records"), (prep, "prepare_records"), (prep, "read_fasta_gpu")],
          "index": [(asgart_amd.Index, "__init__")],
          "search": [(asgart_amd.Index, "search_duplications_passes")],
          "post_process": [(asgart_amd.Index, "post_process")],
          "score": [(asgart_amd.Index, "compute_scores_shard"), (asgart_amd.Index, "compute_scores_flags_shard")]}


class Clock:
    """Wall time spent inside the calls named in PHASES (each ends with its results on the host)."""

    def __init__(self):
        self.t = {k: 0.0 for k in PHASES}
        self.saved = []

    def __enter__(self):
        for phase, targets in PHASES.items():
            for owner, name in targets:
                fn = getattr(owner, name)
                self.saved.append((owner, name, fn))
                setattr(owner, name, self.timed(phase, fn))
        return self

    def timed(self, phase, fn):
        def call(*a, **k):
            t0 = time.perf_counter()
            try:
                out = fn(*a, **k)
                return list(out) if phase == "prepare" and fn.__name__ == "read_records" else out   # (a generator)
            finally:
                self.t[phase] += time.perf_counter() - t0
        return call

    def __exit__(self, *exc):
        for owner, name, fn in self.saved:
            setattr(owner, name, fn)


def timed_run(fn):
    with Clock() as ck:
        t0 = time.perf_counter()
        out = fn()
        wall = time.perf_counter() - t0
    res = {"wall_s": round(wall, 3)}
    res.update({k + "_s": round(v, 3) for k, v in ck.t.items()})
    res["other_s"] = round(wall - sum(ck.t.values()), 3)
    return out, res


def main():
    import torch.distributed as dist

    name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
    toks = sys.argv[2] if len(sys.argv) > 2 else "direct,RC"
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"orientations_{name}.json")
    reader = sys.argv[4] if len(sys.argv) > 4 else None
    cfg, scale = CONFIGS[name]
    orientations = postprocess.parse_orientations(toks)
    base = asgart_amd.RunSettings.from_cli()
    recs = synth.config_genome(cfg, scale)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dist.init_process_group("gloo", rank=0, world_size=1)
    res = {"workload": name, "reader": reader or "device", "orientations": toks.split(","), "bases": int(sum(len(s) for _, s in recs)), "runs": []}
    ok = True
    try:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, f"{name}.fa")
            with open(path, "wb") as fh:
                for rec_name, seq in recs:
                    fh.write(b">" + rec_name.encode() + b"\n" + bytes(seq) + b"\n")
            del recs
            files = [path]
            # warm-up: code objects, allocator pools, the process group
            multi.search_duplications(files, base, dist, 0, compute_score=True, reader=reader)
            for score in (False, True):
                singles, single_t = [], []
                for r, c in orientations:
                    st = replace(base, reverse=r, complement=c)
                    (text, _), t = timed_run(lambda: multi.search_duplications(files, st, dist, 0, compute_score=score,
                                                                                        reader=reader))
                    singles.append(text)
                    single_t.append(t)
                (per, merged), one_t = timed_run(
                    lambda: multi.search_orientations(files, orientations, base, dist, 0, compute_score=score,
                                                      reader=reader))
                same = [text for text, _ in per] == singles
                ok = ok and same
                total = {k: round(sum(t[k] for t in single_t), 3) for k in single_t[0]}
                res["runs"].append({"compute_score": score, "one_run_per_orientation": single_t,
                                    "one_run_per_orientation_total": total, "one_run_over_all": one_t,
                                    "duplications": [text.count('"chr_left": ') for text in singles],
                                    "merged_bytes": len(merged), "identical": same})
    finally:
        dist.destroy_process_group()
    line = json.dumps(res)
    print(line, flush=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
