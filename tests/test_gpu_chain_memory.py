"""asgart_chain_duplications holds no device memory once a call has returned, refused or not: the bounds of
test_gpu_groups_memory.py for the tool that joined them (csrc/chain.hip on tool_base.hpp's ToolWork)."""
import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info)

import asgart_amd
from asgart_amd import chain

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
    """600 anchors over three names, near one diagonal.  The call has no refusal behind its launches."""
    rng = np.random.default_rng(1)
    n = 600
    chr_ = rng.integers(0, 3, 2 * n).astype(np.int32)
    pl = rng.integers(0, 40_000, n)
    pos = np.column_stack([pl, pl + 50 + rng.integers(0, 30, n)]).reshape(-1).astype(np.uint64)
    length = rng.integers(1, 120, 2 * n).astype(np.uint64)
    flags = rng.integers(0, 4, n).astype(np.uint8)
    bad, empty, flag = chr_.copy(), length.copy(), flags.copy()
    bad[10] = 3
    empty[14] = 0
    flag[9] = 4

    def one_round():
        assert "duplication 5 " in _refused(-1, chain.chain_duplications, bad, pos, length, flags, 3)
        assert "duplication 7 " in _refused(-1, chain.chain_duplications, chr_, pos, empty, flags, 3)
        assert "duplication 9 " in _refused(-1, chain.chain_duplications, chr_, pos, length, flag, 3)
        _refused(-1, chain.chain_duplications, chr_, pos, length, flags, 3, lookback=1025)
        _refused(-3, chain.chain_duplications, chr_, pos, length, flags, 3, device=99)
        for lookback in [64, 65] * 10:
            assert chain.chain_duplications(chr_, pos, length, flags, 3, 300, lookback).n_chains > 1

    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]
