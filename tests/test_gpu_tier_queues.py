"""The extension tiers are planned onto the hardware queues a process may open (asgart_tier_plan): results must not
depend on that budget.  Each budget runs in a fresh child process (tests/tier_queues_child.py) under a time limit of its
own: the battery cases bit-exact with the oracle, default and forced placement, and cfg3s and cfg4 against the
committed digests.  Run with `pytest -m gpu` on an MI355X."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT_S = 900


@pytest.mark.parametrize("queues", [2, 4, 8])
def test_results_do_not_depend_on_the_queue_budget(hiplib, queues):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASGART_")}   # shipped defaults, no presets
    env["GPU_MAX_HW_QUEUES"] = str(queues)
    p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(HERE, "tier_queues_child.py")],
                       env=env, capture_output=True, text=True, timeout=LIMIT_S + 60)
    tail = f"exit {p.returncode}\n--- stdout\n{p.stdout[-4000:]}\n--- stderr\n{p.stderr[-4000:]}"
    assert p.returncode == 0, tail
    assert "ALL OK" in p.stdout, tail
    plans = re.findall(r"tier plan \((\d+) tier streams", p.stderr)
    assert plans and all(int(n) == min(6, queues) for n in plans), tail
