"""Child process of tests/test_gpu_run_directory.py: one process with ASGART_RUN_DIR as its parent set it (the variable is
read when an index is created).  asgart_searcher_search for every probe of the test's text, direct and -RC, at every probe
size of the test -> an .npz of (lo, hi) arrays at the path given, and one JSON line: asgart_run_dir_info per probe size."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import asgart_amd  # noqa: E402
import oracle  # noqa: E402
from test_gpu_run_directory import DIRECT, KS, RC, gpu_ranges, make_text  # noqa: E402

if __name__ == "__main__":
    text = make_text()
    sa = oracle.Index.build(text).sa
    ranges, info = {}, {}
    with asgart_amd.Index(text, sa) as idx:
        for k in KS:
            for name, mode in (("direct", DIRECT), ("rc", RC)):
                ranges[f"k{k}_{name}"] = gpu_ranges(idx, text, k, mode)
            info[str(k)] = idx.run_dir_info()
    np.savez(sys.argv[1], **ranges)
    print(json.dumps(info), flush=True)
