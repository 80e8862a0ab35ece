"""The rows and the name keys that rosary.hip, groups.hip and chain.hip take from csrc/tool_base.hpp, where the name table
is as large as the geometry: the row-offsets kernel is one template for uint32_t and int32_t names and its grid is sized
by the names, not by the arms, and the name sorts take ceil(log2(n_names)) bits.  300 duplications (600 arms) on
n_names = block - 1, block, block + 1 and 2 block + 1 names are the smallest inputs at which a grid that is one workgroup
short leaves rows unwritten, or a key one bit short orders the top id among the low ones; with three names neither shows.
Every output array against rosary.clusters_numpy, groups.groups_host and chain.chain_host."""
import dataclasses

import numpy as np
import pytest

from asgart_amd import chain, groups, rosary

pytestmark = pytest.mark.gpu

N_SDS = 300
SPAN = 4_000
PATTERNS = ["every third id", "id 0 and the top id", "the top id"]


def names_around(block):
    return [block - 1, block, block + 1, 2 * block + 1]


def ids_of(pattern, n_names):
    return {"every third id": list(range(0, n_names, 3)), "id 0 and the top id": [0, n_names - 1],
            "the top id": [n_names - 1]}[pattern]


def arms(seed, ids):
    """600 arms on the given name ids in a span of 4 000, lengths 1 .. 64, and a flag byte per duplication."""
    rng = np.random.default_rng(seed)
    m = 2 * N_SDS
    return (rng.choice(ids, size=m).astype(np.int32), rng.integers(0, SPAN, size=m).astype(np.uint64),
            rng.integers(1, 65, size=m).astype(np.uint64), rng.integers(0, 4, size=N_SDS).astype(np.uint8))


def assert_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert (got == want).all(), (what, np.flatnonzero(got != want)[:5].tolist())


@pytest.mark.parametrize("pattern", PATTERNS)
def test_rosary_rows_where_the_names_fill_the_geometry(hiplib, pattern):
    block = rosary.rosary_geometry()
    for n_names in names_around(block):
        name, start, length, flags = arms(n_names, ids_of(pattern, n_names))
        got = rosary.rosary_clusters(name, start, length, flags, 37, n_names)
        want = rosary.clusters_numpy(name, start, length, flags, 37, n_names)
        for field, g, w in zip(("name_offsets", "start", "length", "klass", "members"), got, want):
            assert_equal(g, w, (n_names, field))
        assert len(got[0]) == n_names + 1 and got[0][-1] == len(got[1])


@pytest.mark.parametrize("pattern", PATTERNS)
def test_groups_rows_where_the_names_fill_the_geometry(hiplib, pattern):
    block = groups.groups_geometry()
    for n_names in names_around(block):
        name, start, length, _ = arms(n_names + 1, ids_of(pattern, n_names))
        got = groups.duplication_groups(name, start, length, 37, n_names)
        want = groups.groups_host(name, start, length, 37, n_names)
        for f in dataclasses.fields(groups.Groups):
            assert_equal(getattr(got, f.name), getattr(want, f.name), (n_names, f.name))
        assert len(got.name_offsets) == n_names + 1 and got.name_offsets[-1] == got.n_loci


@pytest.mark.parametrize("lookback", [1, 64])
def test_chains_of_anchors_on_the_top_two_names(hiplib, lookback):
    """The packed group key holds cl and cr in ceil(log2(n_names)) bits each, cr above the two flag bits and cl above cr:
    in a field one bit short the top id of block + 1 and of 2 block + 1 names reaches into its neighbour."""
    block = chain.chain_geometry()[0]
    links = 0
    for n_names in names_around(block):
        rng = np.random.default_rng(n_names + lookback)
        span = 40 * N_SDS + 100
        fl = rng.integers(0, 4, N_SDS).astype(np.uint8)
        pl = rng.integers(0, span, N_SDS)
        pr = np.where(fl & 1, span + 40 - pl, pl + 40) + rng.integers(-25, 26, N_SDS)   # near one diagonal per orientation
        args = (rng.choice([n_names - 2, n_names - 1], size=2 * N_SDS).astype(np.int32),
                np.column_stack([pl, pr]).reshape(-1).astype(np.uint64), rng.integers(1, 120, 2 * N_SDS).astype(np.uint64), fl)
        got = chain.chain_duplications(*args, n_names, 300, lookback)
        want = chain.chain_host(*args, n_names, 300, lookback)
        for f in dataclasses.fields(chain.Chains):
            assert_equal(getattr(got, f.name), getattr(want, f.name), (n_names, f.name))
        links += got.n_links
    assert links > 20
