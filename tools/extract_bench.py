"""The duplicons' sequences of a whole run, on the GPU (asgart_amd.Source: asgart_extract_sequences) against a numpy
gather of the same arms on the host (the reference's per-duplication slice, reverse and complement,
src/bin/asgart-extract.rs:110-131), for the surviving duplications of every pass of a bench workload.

    python tools/extract_bench.py [cfg4] [out.json]

Prints one JSON line (and writes it to out.json): per pass the duplications, the bytes extracted, the GPU time of the
first and of a second extraction (host buffer to host buffer, the copies included) and the numpy time; the upload of the
raw records (Source.from_records) is timed on its own.  The two outputs are compared byte for byte.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import asgart_amd  # noqa: E402
from asgart_amd import postprocess, prep, synth  # noqa: E402

COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ATGCNatgcn", b"TACGNtacgn"):
    COMP[_a] = _b

CONFIGS = {"cfg4": (4, 1.0, False), "cfg3": (3, 1.0, True), "tiny": (2, 0.05, False)}


def numpy_gather(src, sds, rev, comp):
    """-> (ends, bytes) as Source.extract returns them, one duplication at a time on the host."""
    lens = sds[:, 2:4].astype(np.int64).reshape(-1)
    ends = np.cumsum(lens)
    out = np.empty(int(ends[-1]) if len(ends) else 0, dtype=np.uint8)
    o = 0
    for (l, r, ll, rl) in sds.astype(np.int64).tolist():
        out[o:o + ll] = src[l:l + ll]
        o += ll
        right = src[r:r + rl]
        if rev:
            right = right[::-1]
        out[o:o + rl] = COMP[right] if comp else right
        o += rl
    return ends.astype(np.uint64), out


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    cfg, scale, skip_masked = CONFIGS[name]
    t0 = time.perf_counter()
    recs = synth.config_genome(cfg, scale)
    gen_s = time.perf_counter() - t0
    pr, idx = prep.prepare_records_gpu(recs, skip_masked=skip_masked, want_text=False)
    modes = ((False, False), (True, True))
    sts = [asgart_amd.RunSettings.from_cli(reverse=r, complement=c, skip_masked=skip_masked) for r, c in modes]
    with idx:
        idx.prepare(20)
        raw = idx.search_duplications_passes(pr.chunks, sts)
        post = [postprocess.post_process_arrays(idx, o, s)[1] for o, s in raw]
    t0 = time.perf_counter()
    src_gpu = asgart_amd.Source.from_records(recs, 0)
    upload_s = time.perf_counter() - t0
    src = np.concatenate([np.asarray(s, dtype=np.uint8) for _, s in recs])
    res = {"workload": name, "source_bytes": int(len(src)), "generate_s": round(gen_s, 1),
           "source_upload_s": round(upload_s, 3), "passes": []}
    with src_gpu:
        for (r, c), sds in zip(modes, post):
            t0 = time.perf_counter()
            ends, data = src_gpu.extract(sds, r, c)
            first = time.perf_counter() - t0
            t0 = time.perf_counter()
            ends, data = src_gpu.extract(sds, r, c)
            second = time.perf_counter() - t0
            t0 = time.perf_counter()
            h_ends, h_data = numpy_gather(src, sds, r, c)
            host = time.perf_counter() - t0
            same = bool(np.array_equal(ends, h_ends) and np.array_equal(data, h_data))
            res["passes"].append({"reverse": r, "complement": c, "duplications": int(len(sds)), "bytes": int(len(data)),
                                  "gpu_first_s": round(first, 4), "gpu_s": round(second, 4),
                                  "gpu_GBps": round(len(data) / second / 1e9, 2) if second > 0 else None,
                                  "numpy_s": round(host, 3), "identical": same})
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(p["identical"] for p in res["passes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
