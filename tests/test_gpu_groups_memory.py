"""asgart_duplication_groups holds no device memory once a call has returned, refused or not: the bounds of
test_gpu_tools_memory.py for the tool that joined them (csrc/groups.hip on tool_base.hpp's ToolWork)."""
import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info)

import asgart_amd
from asgart_amd import groups

pytestmark = pytest.mark.gpu


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _refused(code, call, *args, **kwargs):
    with pytest.raises(asgart_amd.AsgartError) as e:
        call(*args, **kwargs)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusals_and_repeated_calls_leave_no_device_memory(hiplib):
    """300 duplications (600 arms) over three names.  The call has no refusal behind its launches."""
    rng = np.random.default_rng(1)
    name = rng.integers(0, 3, 600).astype(np.int32)
    start = rng.integers(0, 40_000, 600).astype(np.uint64)
    length = rng.integers(1, 65, 600).astype(np.uint64)
    bad, empty = name.copy(), length.copy()
    bad[5] = 3
    empty[7] = 0

    def one_round():
        assert "arm 5 " in _refused(-1, groups.duplication_groups, bad, start, length, 37, 3)
        assert "arm 7 " in _refused(-1, groups.duplication_groups, name, start, empty, 37, 3)
        _refused(-3, groups.duplication_groups, name, start, length, 37, 3, device=99)
        for _ in range(20):
            assert groups.duplication_groups(name, start, length, 37, 3).n_groups > 1

    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]
