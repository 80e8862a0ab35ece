"""The device work the result tools share (csrc/tool_base.hpp: ToolWork) gives back what a call took: slice, plot and rosary,
like test_refusals_and_repeated_calls_leave_no_device_memory of test_gpu_export.py for export, with its bounds."""
import numpy as np
import pytest
import torch  # (before the library loads the HIP runtime: torch.cuda.mem_get_info)

import asgart_amd
from asgart_amd import plot, rosary
from asgart_amd import slice as sl
from test_gpu_plot import OPEN, P, random_arrays, random_tracks
from test_gpu_rosary import random_arms
from test_gpu_slice import plain_plan, rows

pytestmark = pytest.mark.gpu


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _refused(code, call, *args, **kwargs):
    with pytest.raises(asgart_amd.AsgartError) as e:
        call(*args, **kwargs)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def _slice_round():
    """600 duplications; the last 300 have their right arm on a name the map does not hold."""
    sds, flags, chr_, pos = rows(600, 8)
    chr_[:] = 0
    chr_[300:, 1] = 2
    sp = plain_plan(n_names=3, exclude=1, relocate=1, drop_empty=1)
    sp.exclude = np.array([0, 3, 4], np.uint8)               # n1 excluded, n2 not in the map
    sp.final_pos = np.array([0, -1, -1], np.int64)
    good = chr_.copy()
    good[300:, 0] = 1                                        # every such duplication is excluded itself
    bad = good.copy()
    bad[7, 1] = 3

    def one_round():
        assert "duplication 7 has name id 3" in _refused(-1, sl.slice_families, [0, 600], sds, flags, bad, pos, sp)
        _refused(-3, sl.slice_families, [0, 600], sds, flags, good, pos, sp, device=99)
        # after the stages ran: every buffer but the outputs is allocated when the error ordinal is read back
        assert "duplication 300 passes the exclusion" in _refused(-1, sl.slice_families, [0, 600], sds, flags, chr_, pos, sp)
        for _ in range(20):
            assert sl.slice_families([0, 600], sds, flags, good, pos, sp)[5].tolist() == list(range(300))
    return one_round


def _plot_round():
    """448 duplications in families of 0 .. 255 and 300 positions; for the refusal five positions, which leave most
    duplications without a match, and behind them one on a fragment the map does not hold.  asgart_plot_filter takes no name
    ids: its refusal before the launch is an offset array that decreases."""
    arr = random_arrays(2, [0, 1, 63, 64, 65, 255])
    assert arr.n == 448
    tracks = random_tracks(3, 300)
    sparse = random_tracks(4, 5) + [[{"name": "lost", "positions": [{"chr": "nowhere", "start": 1, "length": 1}]}]]
    ta = plot.resolve_tracks(arr._strand_dict()["map"], tracks)
    offs = np.array(arr.offs)
    offs[2] = offs[3] + 1

    def one_round():
        assert "fam_offsets decrease" in _refused(-1, plot.plot_filter, offs, arr.sds, arr.identity, ta,
                                                  plot._c_options(P(**OPEN)))
        _refused(-3, plot.apply_arrays, arr, tracks, P(filter_duplicons=5, **OPEN), device=99)
        # after the join of filter_duplicons: a duplication that matched nothing reaches the unresolved position
        with pytest.raises(ValueError, match="Unable to find fragment `nowhere`"):
            plot.apply_arrays(arr, sparse, P(filter_duplicons=0, **OPEN))
        for _ in range(20):
            got, _ = plot.apply_arrays(arr, tracks, P(filter_duplicons=5, filter_features=5, **OPEN))
            assert 0 < got.n < arr.n
    return one_round


def _rosary_round():
    """300 duplications (600 arms) over three names.  asgart_rosary_clusters has no refusal behind its launches."""
    name, start, length, flags = random_arms(1, 600, 3)
    bad = name.copy()
    bad[5] = 3

    def one_round():
        assert "arm 5 " in _refused(-1, rosary.rosary_clusters, bad, start, length, flags, 37, 3)
        _refused(-3, rosary.rosary_clusters, name, start, length, flags, 37, 3, device=99)
        for _ in range(20):
            assert len(rosary.rosary_clusters(name, start, length, flags, 37, 3)[1]) > 0
    return one_round


@pytest.mark.parametrize("tool", ["slice", "plot", "rosary"])
def test_refusals_and_repeated_calls_leave_no_device_memory(hiplib, tool):
    one_round = {"slice": _slice_round, "plot": _plot_round, "rosary": _rosary_round}[tool]()
    asgart_amd.trim_cache(0)
    after = [_free_bytes()]
    for rep in range(2):
        one_round()
        asgart_amd.trim_cache(0)
        after.append(_free_bytes())
    assert after[1] - after[2] <= (1 << 20), [x - after[0] for x in after]
    assert after[0] - after[2] <= (256 << 20), [x - after[0] for x in after]
