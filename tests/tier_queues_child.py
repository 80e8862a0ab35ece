"""Child process of tests/test_gpu_tier_queues.py: one process with the hardware-queue budget its parent put into
GPU_MAX_HW_QUEUES.  Every battery case in two orientations, as single calls and as one passes call, once with the
default placement and once with every segment forced into the workgroup tiers (all tier streams busy), bit-exact with
the oracle; then the passes call of cfg3s and cfg4 three times each against the committed digests.  Prints the tier
plan of one call (option debug) on stderr and "ALL OK" at the end."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import pytest  # noqa: E402

import asgart_amd  # noqa: E402
import oracle  # noqa: E402
from test_gpu_options import _check_three_calls_shipped_defaults, _same, _what  # noqa: E402
from test_gpu_parity import BATTERY, _battery_case  # noqa: E402

ORIENTATIONS = ((False, False), (True, True))


def battery():
    for name in sorted(BATTERY):
        pr, cli = _battery_case(name)
        oidx = oracle.Index.build(pr.data)
        sts = [asgart_amd.RunSettings.from_cli(reverse=r, complement=c, **cli) for r, c in ORIENTATIONS]
        exp = [oidx.run_raw(pr.chunks, oracle.make_settings(reverse=r, complement=c, **cli), threads=4)
               for r, c in ORIENTATIONS]
        with asgart_amd.Index(pr.data, oidx.sa) as idx:
            for force in (0, 6):
                idx.set_option("force_tier", force)
                if name == "dense_repeats" and force == 6:
                    idx.set_option("debug", 1)   # (the plan of this call goes to stderr)
                for st, e, m in zip(sts, exp, ORIENTATIONS):
                    got = idx.search_duplications_raw(pr.chunks, st)
                    assert _same(got, e), (name, force, m, "single", _what(got, e))
                idx.set_option("debug", 0)
                for got, e, m in zip(idx.search_duplications_passes(pr.chunks, sts), exp, ORIENTATIONS):
                    assert _same(got, e), (name, force, m, "passes", _what(got, e))
        print(f"{name}: bit-exact", flush=True)


if __name__ == "__main__":
    print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}", flush=True)
    battery()
    mp = pytest.MonkeyPatch()
    try:
        for cfg in ("cfg3s", "cfg4"):
            _check_three_calls_shipped_defaults(cfg, mp)
            print(f"{cfg}: three calls match the committed digests", flush=True)
    finally:
        mp.undo()
    print("ALL OK", flush=True)
