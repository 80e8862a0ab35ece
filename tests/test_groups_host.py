"""groups.groups_host, the readable statement of the paralogy groups (include/asgart_hip.h: loci by the running maximum,
groups by the duplications), against a brute force written here: all pairs of arms for the neighbour relation, DFS over the
arms, DFS over the loci and edges.  The cases the rule names, regroup through the result forms, the three writers against
literal text, and every refusal with its message.  No GPU."""
import dataclasses

import numpy as np
import pytest

from asgart_amd import groups, rosary
from asgart_amd.slice import ResultArrays

M64 = 2 ** 64 - 1
SPAN = 4_000
MARGINS = [0, 37, M64]
SETTINGS = {"probe_size": 20, "max_gap_size": 120, "min_duplication_length": 1000, "max_cardinality": 500, "trim": None,
            "skip_masked": False}


def random_arms(seed, m, n_names):
    """m arms over n_names names in a span of 4 000, lengths 1 .. 64; with 3 names one has no arm, with 70 three have none."""
    rng = np.random.default_rng(seed)
    ids = {1: [0], 3: [k for k in range(3) if k != seed % 3], 70: [k for k in range(70) if k not in (0, 35, 69)]}[n_names]
    return (rng.choice(ids, size=m).astype(np.int32), rng.integers(0, SPAN, size=m).astype(np.uint64),
            rng.integers(1, 65, size=m).astype(np.uint64))


def components(n, neighbours):
    """Labels of the connected components of n nodes, numbered by their smallest node; neighbours: adjacency lists."""
    label = [-1] * n
    count = 0
    for root in range(n):
        if label[root] >= 0:
            continue
        stack = [root]
        label[root] = count
        while stack:
            x = stack.pop()
            for y in neighbours[x]:
                if label[y] < 0:
                    label[y] = count
                    stack.append(y)
        count += 1
    return label, count


def brute(name, start, length, margin, n_names):
    """The rule by its definitions: the neighbour relation on all pairs, components of arms, then of loci."""
    name, start, length = [np.asarray(v).tolist() for v in (name, start, length)]
    m = len(name)
    end = [s + ln for s, ln in zip(start, length)]

    def sat(x):
        return min(x + margin, M64)

    near = [[b for b in range(m) if name[a] == name[b] and start[a] < sat(end[b]) and start[b] < sat(end[a])]
            for a in range(m)]
    comp, n_comp = components(m, near)
    # the loci in (name, start) order
    by_comp = [[j for j in range(m) if comp[j] == c] for c in range(n_comp)]
    by_comp.sort(key=lambda arms: (name[arms[0]], min(start[j] for j in arms)))
    arm_locus = [0] * m
    for x, arms in enumerate(by_comp):
        for j in arms:
            arm_locus[j] = x
    l_name = [name[arms[0]] for arms in by_comp]
    l_start = [min(start[j] for j in arms) for arms in by_comp]
    l_length = [max(end[j] for j in arms) - s for arms, s in zip(by_comp, l_start)]
    links = [[] for _ in by_comp]
    for q in range(m // 2):
        a, b = arm_locus[2 * q], arm_locus[2 * q + 1]
        links[a].append(b)
        links[b].append(a)
    l_group, n_groups = components(len(by_comp), links)   # roots ascend: numbered by the smallest locus
    group = [l_group[arm_locus[2 * q]] for q in range(m // 2)]
    order = sorted(range(m // 2), key=lambda q: group[q])
    g_dups = [group.count(g) for g in range(n_groups)]
    return groups.Groups(
        np.array([sum(1 for v in l_name if v < k) for k in range(n_names + 1)], np.int64), np.array(l_name, np.int32),
        np.array(l_start, np.uint64), np.array(l_length, np.uint64), np.array([len(arms) for arms in by_comp], np.uint32),
        np.array(l_group, np.uint32), np.array([l_group.count(g) for g in range(n_groups)], np.uint32),
        np.array(g_dups, np.uint32),
        np.array([sum(ln for ln, g2 in zip(l_length, l_group) if g2 == g) & M64 for g in range(n_groups)], np.uint64),
        np.array(group, np.uint32), np.array(order, np.int64), np.array(np.cumsum([0] + g_dups), np.int64),
        np.array(arm_locus, np.uint32))


def assert_same(got, want):
    for f in dataclasses.fields(groups.Groups):
        g, w = getattr(got, f.name), getattr(want, f.name)
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), f.name


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("n_names", [1, 3, 70])
@pytest.mark.parametrize("m", [2, 10, 64, 300])
def test_random_arms_against_the_brute_force(m, n_names, margin):
    args = random_arms(1000 * m + n_names, m, n_names)
    assert_same(groups.groups_host(*args, margin, n_names), brute(*args, margin, n_names))


def test_no_arms():
    g = groups.groups_host(np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), 5, 4)
    assert g.name_offsets.tolist() == [0] * 5 and g.group_offsets.tolist() == [0]
    assert g.n_loci == 0 and g.n_groups == 0 and len(g.arm_locus) == 0 and g.order.dtype == np.int64


def test_a_long_arm_holds_the_short_ones_behind_it_where_the_rosary_cuts():
    start = np.array([0, 10, 30, 500, 999, 5000], np.uint64)
    length = np.array([1000, 10, 10, 100, 201, 1], np.uint64)
    name = np.zeros(6, np.int32)
    g = groups.groups_host(name, start, length, 0, 1)
    assert g.arm_locus.tolist() == [0, 0, 0, 0, 0, 1]
    assert (g.locus_start[0], g.locus_length[0], g.locus_members[0]) == (0, 1200, 5)
    # the reference's clusters end where their LAST member ends: after [10, 20) the cluster ends at 20, and 30 > 20 is a cut
    _, c_start, c_length, _, members = rosary.clusters_numpy(name[:5], start[:5], length[:5], None, 0, 1)
    assert c_start.tolist() == [0, 30, 500, 999] and c_length.tolist() == [20, 10, 100, 201]
    assert members.tolist() == [2, 1, 1, 1]
    assert_same(g, brute(name, start, length, 0, 1))


def test_abutting_arms():
    args = (np.zeros(2, np.int32), np.array([0, 10], np.uint64), np.array([10, 5], np.uint64))
    assert groups.groups_host(*args, 0, 1).n_loci == 2
    one = groups.groups_host(*args, 1, 1)
    assert one.n_loci == 1 and one.locus_length.tolist() == [15] and one.group_loci.tolist() == [1]


def test_the_running_maximum_stops_at_a_name():
    g = groups.groups_host([0, 1], [0, 5], [10 ** 9, 5], 0, 2)
    assert g.n_loci == 2 and g.locus_name.tolist() == [0, 1] and g.locus_start.tolist() == [0, 5]
    assert g.name_offsets.tolist() == [0, 1, 2] and g.n_groups == 1 and g.group_bases.tolist() == [10 ** 9 + 5]


def test_self_edges_and_parallel_edges():
    # loci: A [0,10) B [100,110) C [200,210); duplications: A-A (tandem), A-B, A-B again, B-A, C-C
    name = np.zeros(10, np.int32)
    start = np.array([0, 5, 0, 100, 2, 101, 100, 3, 200, 205], np.uint64)
    length = np.array([5, 5, 10, 10, 3, 9, 5, 2, 6, 5], np.uint64)
    g = groups.groups_host(name, start, length, 0, 1)
    assert g.arm_locus.tolist() == [0, 0, 0, 1, 0, 1, 1, 0, 2, 2]
    assert g.locus_group.tolist() == [0, 0, 1] and g.group.tolist() == [0, 0, 0, 0, 1]
    assert g.group_loci.tolist() == [2, 1] and g.group_duplications.tolist() == [4, 1]
    assert g.group_bases.tolist() == [20, 10] and g.group_offsets.tolist() == [0, 4, 5]
    assert_same(g, brute(name, start, length, 0, 1))


def test_groups_are_numbered_by_their_smallest_locus():
    # loci 0 .. 5 at 0, 100, ...; edges 5-1, 4-2, 3-3, 0-4: groups {0, 2, 4}, {1, 5}, {3}
    pairs = [(5, 1), (4, 2), (3, 3), (0, 4)]
    start = np.array([100 * x for pair in pairs for x in pair], np.uint64)
    g = groups.groups_host(np.zeros(8, np.int32), start, np.full(8, 10, np.uint64), 0, 1)
    assert g.locus_group.tolist() == [0, 1, 0, 2, 0, 1]
    assert g.group.tolist() == [1, 0, 2, 0] and g.order.tolist() == [1, 3, 0, 2] and g.group_offsets.tolist() == [0, 2, 3, 4]
    assert g.group_loci.tolist() == [3, 2, 1] and g.group_duplications.tolist() == [2, 1, 1]


def hand_made():
    """Three fragments (the last without a duplication, of length 0), four duplications in three families."""
    def sd(cl, pl, ll, cr, pr, rl, ident, rev=False):
        base = {"chrA": 0, "chrB": 1000, "empty": 3000}
        return {"chr_left": cl, "chr_right": cr, "global_left_position": base[cl] + pl,
                "global_right_position": base[cr] + pr, "chr_left_position": pl, "chr_right_position": pr,
                "left_length": ll, "right_length": rl, "left_seq": None, "right_seq": None,
                "identity": np.float32(ident), "reversed": rev, "complemented": rev}
    return {"strand": {"name": "hand", "length": 3000,
                       "map": [{"name": "chrA", "position": 0, "length": 1000},
                               {"name": "chrB", "position": 1000, "length": 2000},
                               {"name": "empty", "position": 3000, "length": 0}]},
            "settings": dict(SETTINGS, reverse=True, complement=True),
            "families": [[sd("chrB", 500, 100, "chrB", 1500, 100, float("nan"))],
                         [sd("chrA", 100, 50, "chrB", 40, 50, 0.5), sd("chrA", 120, 60, "chrA", 400, 60, 97.25, True)],
                         [sd("chrB", 60, 40, "chrA", 420, 10, 1.0)]]}


def test_regroup_round_trips_and_is_idempotent():
    a = ResultArrays.from_result(hand_made())
    g = groups.Groups.from_arrays(a, 0, host=True)
    # loci: chrA [100,180) [400,460); chrB [40,100) [500,600) [1500,1600); groups {0, 1, 2} and {3, 4}
    assert g.locus_group.tolist() == [0, 0, 0, 1, 1] and g.order.tolist() == [1, 2, 3, 0]
    b = groups.regroup(a, g)
    assert b.offs.tolist() == [0, 3, 4] and b.names == a.names and b.settings == a.settings
    assert (b.map_name == a.map_name).all() and b.strand_name == a.strand_name
    back = ResultArrays.from_result(b.to_result())
    for field in ("offs", "sds", "flags", "chr", "chr_pos", "map_name", "map_pos", "map_len"):
        assert (getattr(back, field) == getattr(b, field)).all(), field
    assert back.identity.tobytes() == b.identity.tobytes()

    def rows(x):
        return sorted(zip(x.sds.tolist(), x.flags.tolist(), x.chr.tolist(), x.chr_pos.tolist(),
                          x.identity.view(np.uint32).tolist()))
    assert rows(a) == rows(b)
    g2 = groups.Groups.from_arrays(b, 0, host=True)
    assert g2.order.tolist() == [0, 1, 2, 3] and (g2.group_offsets == g.group_offsets).all()
    c = groups.regroup(b, g2)
    for field in ("offs", "sds", "flags", "chr", "chr_pos"):
        assert (getattr(c, field) == getattr(b, field)).all(), field
    assert c.identity.tobytes() == b.identity.tobytes()
    with pytest.raises(ValueError, match="regroup: the groups are of 4 duplications, the result has 3"):
        groups.regroup(ResultArrays.from_result(dict(hand_made(), families=hand_made()["families"][1:])), g)


def test_the_writers_on_a_hand_made_result():
    a = ResultArrays.from_result(hand_made())
    g = groups.Groups.from_arrays(a, 0, host=True)
    assert groups.loci_text(a, g) == (
        "#name\tstart\tend\tlocus\tmembers\tstrand\tgroup\tcopies\tgroup_bases\n"
        "chrA\t100\t180\tL0\t2\t.\t0\t3\t200\n"
        "chrA\t400\t460\tL1\t2\t.\t0\t3\t200\n"
        "chrB\t40\t100\tL2\t2\t.\t0\t3\t200\n"
        "chrB\t500\t600\tL3\t1\t.\t1\t2\t200\n"
        "chrB\t1500\t1600\tL4\t1\t.\t1\t2\t200\n")
    assert groups.groups_text(a, g) == (
        "#group\tloci\tduplications\tbases\tnames\tmin_identity\tmax_identity\n"
        "0\t3\t3\t200\t2\t0.5\t97.25\n"
        "1\t2\t1\t200\t1\t.\t.\n")
    assert groups.fragments_text(a, g) == (
        "#name\tlength\tloci\tduplicated_bases\tfraction\n"
        "chrA\t1000\t2\t140\t0.14\n"
        "chrB\t2000\t3\t260\t0.13\n"
        "empty\t0\t0\t0\t.\n"
        "#total\t3000\t5\t400\t0.13333333333333333\n")


def test_members_are_capped_in_the_bed_score():
    n = 1001   # 2002 arms on one spot
    a = ResultArrays("s", 10, SETTINGS, ["c"], [0], [0], [10], [0, n], np.tile(np.array([0, 0, 5, 5], np.uint64), (n, 1)),
                     np.zeros(n, np.uint8), np.zeros((n, 2), np.int32), np.zeros((n, 2), np.uint64), np.zeros(n, np.float32))
    g = groups.Groups.from_arrays(a, 0, host=True)
    assert g.locus_members.tolist() == [2002]
    assert groups.loci_text(a, g).splitlines()[1] == "c\t0\t5\tL0\t1000\t.\t0\t1\t5"
    assert groups.groups_text(a, g).splitlines()[1] == "0\t1\t1001\t5\t1\t0\t0"


def test_refusals_name_the_first_offender():
    ok = ([0, 1, 1, 0], [0, 5, 7, 9], [4, 4, 4, 4])

    def refused(name, start, length, margin=0, n_names=2):
        with pytest.raises(ValueError) as e:
            groups.groups_host(name, start, length, margin, n_names)
        return str(e.value)

    assert groups.groups_host(*ok, 0, 2).n_loci == 3
    assert refused([0, 1, 2, 3], *ok[1:]) == "groups_host: arm 2 (duplication 1, left) has the name id 2, outside [0, 2)"
    assert refused([0, -1, 1, 0], *ok[1:]) == "groups_host: arm 1 (duplication 0, right) has the name id -1, outside [0, 2)"
    assert refused(ok[0], ok[1], [4, 4, 4, 0]) == ("groups_host: arm 3 (duplication 1, right) has length 0: an empty arm "
                                                   "belongs to no locus")
    assert refused(ok[0], [0, M64, 7, 9], [4, 1, 0, 4]) == (f"groups_host: arm 1 (duplication 0, right): start {M64} + "
                                                            "length 1 wraps past 2^64")
    assert groups.groups_host(ok[0], [0, M64 - 1, 7, 9], [4, 1, 4, 4], 0, 2).locus_length.tolist() == [4, 4, 4, 1]
    assert refused(*ok, n_names=-1) == "groups_host: a negative count (n_sds = 2, n_names = -1)"
    assert refused([0, 1, 1], [0, 5, 7], [4, 4, 4]) == "groups_host: two arms per duplication, the arrays differ in length"
    assert refused(ok[0], ok[1], [4, 4, 4]) == "groups_host: two arms per duplication, the arrays differ in length"
    assert refused(*ok, margin=M64 + 1) == "--margin is u64"
    assert refused(*ok, margin=-1) == "--margin is u64"
