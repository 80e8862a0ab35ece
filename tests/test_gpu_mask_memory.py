"""asgart_mask_intervals and asgart_fasta_write give back what a call took, like the tools of test_gpu_tools_memory.py, with
its bounds: refusals before the launch, a device that is not there, and repeated calls leave no device memory (the source
a writer reads is the caller's, and is closed inside the round)."""
import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info)

import asgart_amd
from asgart_amd import mask

pytestmark = pytest.mark.gpu


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _refused(code, call, *args, **kwargs):
    with pytest.raises(asgart_amd.AsgartError) as e:
        call(*args, **kwargs)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def _sweep_round():
    """3 000 arms on two records of 200 000 bases."""
    rng = np.random.default_rng(1)
    rs, rl = np.array([0, 200_000], np.uint64), np.array([200_000, 200_000], np.uint64)
    rec = rng.integers(0, 2, 3000).astype(np.int32)
    st = rng.integers(0, 190_000, 3000).astype(np.uint64)
    ln = rng.integers(1, 5000, 3000).astype(np.uint64)
    bad = ln.copy()
    bad[5] = 0

    def one_round():
        assert "arm 5 has length 0" in _refused(-1, mask.mask_intervals, rec, st, bad, rs, rl)
        _refused(-3, mask.mask_intervals, rec, st, ln, rs, rl, device=99)
        for _ in range(20):
            assert mask.mask_intervals(rec, st, ln, rs, rl, 10, 2).n > 0
    return one_round


def _writer_round():
    """Two records of 200 000 bases, 300 intervals: a file of 400 kB."""
    rng = np.random.default_rng(2)
    records = [rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), 200_000) for _ in range(2)]
    rs, rl = np.array([0, 200_000], np.uint64), np.array([200_000, 200_000], np.uint64)
    iv = np.sort(rng.choice(400_000, 600, replace=False)).reshape(-1, 2).astype(np.uint64)
    headers = [b">one", b">two"]

    def one_round():
        with asgart_amd.Source.from_records(records) as src:
            assert "interval 0" in _refused(-1, mask.write_fasta_gpu, src, rs, rl, headers, [(5, 5)], 60, 0)
            assert "holds a line end" in _refused(-1, mask.write_fasta_gpu, src, rs, rl, [b">one", b">t\no"], iv, 60, 0)
            for _ in range(20):
                assert len(mask.write_fasta_gpu(src, rs, rl, headers, iv, 60, 0)) == 400_000 + 2 * 3334 + 10
    return one_round


@pytest.mark.parametrize("call", ["sweep", "writer"])
def test_refusals_and_repeated_calls_leave_no_device_memory(hiplib, call):
    one_round = {"sweep": _sweep_round, "writer": _writer_round}[call]()
    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]
