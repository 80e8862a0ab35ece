"""Child process of tests/test_gpu_tail_up.py: one process with the hardware-queue budget its parent put into
GPU_MAX_HW_QUEUES.  The two array cases, both orientations as single calls and as one passes call, with the tail rule off,
on, and in its shipped default mode 1 (on where the call has fewer tier streams than arm-resident tiers; threshold = the
hits of the array's segment each time), bit-exact with the oracle.  Prints the tier plan of one call (option
debug) on stderr and one JSON line: per case and setting the digest of every result (families, ProtoSDs, keys) and the
per-tier segment counts."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import asgart_amd  # noqa: E402
from test_gpu_tail_up import ARRAYS, _settings, array_case, check_against, digest, run_all  # noqa: E402

if __name__ == "__main__":
    print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}", flush=True)
    out = {}
    for name in sorted(ARRAYS):
        pr, oidx, exp, hits = array_case(name)
        sts = _settings()
        out[name] = {}
        with asgart_amd.Index(pr.data, oidx.sa) as idx:
            idx.set_option("fuse_passes", 2)
            for tag, mode in (("off", 0), ("on", 2), ("default", 1)):
                idx.set_tail_up(mode, hits)
                if tag == "on":
                    idx.set_option("debug", 1)   # (the plan of this call goes to stderr)
                    idx.search_duplications_raw(pr.chunks, sts[0])
                    idx.set_option("debug", 0)
                got, tiers = run_all(idx, pr.chunks, sts)
                check_against(got, exp, None, (name, tag))
                out[name][tag] = {"digest": digest(got), "moved": [m for _, m in tiers],
                                  "tiers": [[int(v) for v in n] for n, _ in tiers]}
    print(json.dumps(out), flush=True)
