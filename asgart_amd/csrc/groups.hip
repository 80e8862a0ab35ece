// groups.hip -- paralogy groups: the arms of a result merged into disjoint loci, the loci linked by the duplications into
// connected components, copy numbers and non-redundant bases per group: asgart_duplication_groups and its handle.  The rule
// is stated once, in include/asgart_hip.h; asgart_amd/groups.py: groups_host is the readable statement of it.
//
// Nothing of the reference does this.  rosary.hip next door restates the reference's clusters, where an arm is compared with
// the END OF THE ARM IN FRONT OF IT; here an arm is compared with the LARGEST end of all arms in front of it (an interval
// union), which needs a scan where rosary needs a neighbour, and the two arms of a duplication are linked, which needs a
// union-find.  What is shared is tool_base.hpp: the ordering, the name offsets and the host tail are the ones of rosary.hip.
//
// Stages, all on one stream; two counts and one give-up word are read back at the very end:
//   emit, sort   the arm ordinals 0 .. 2n - 1 sorted by the 64-bit start, then stably by the name bits (rocPRIM radix sorts,
//                only the ordinal moves); with positive lengths the loci do not depend on how ties are ordered
//   ends         sorted record i: (name, end = start + length), and the start
//   scan         SEGMENTED inclusive max-scan of the ends through rocPRIM's scan: the operator on (name, end) pairs keeps the
//                right name and the larger end where the names agree.  It is associative on a sequence whose names never
//                decrease, which the sort gives.  sat(x + margin) is monotone in x, so the plain ends are scanned
//   heads        head[i] = first of its name || start[i] >= sat(run[i - 1] + margin); the plus-scan of the heads numbers
//                the loci
//   open, close  a head writes name and start and its own slot; the last member writes length = run[i] - start and
//                members = its slot + 1 - the head's; every record scatters its locus to arm_locus in flatten order
//   union        union-find over the loci, a thread per duplication: find with path halving, the LARGER root hooked under
//                the smaller with atomicCAS.  parent[x] <= x always and only ever decreases, so a component's final root is
//                its smallest locus whatever order the threads arrive in.  No lane waits for another lane's store: a walk
//                goes down strictly decreasing indices (at most `arms` steps), a CAS fails only when another lane's hook of
//                the same root succeeded (at most `arms` times in all); both loops carry that bound and a give-up bit that
//                fails the call with a message.  (Built instead of rounds of min-label hooking under a host loop: a fixed
//                number of launches, no read-back per round, and a path of a million loci needs no more of them than a
//                star.)  The duplications go in three launches -- one in 64, then one in 8, then the rest -- with a pass
//                between them that points every locus at its root: with one large group, the usual result, most lanes
//                of the larger launches find ONE parent for their two loci in two loads and leave, without an atomic
//                and without a read of the root's own slot, which every lane of the group would otherwise share
//   flatten      root[x] of every locus (the parents are only read to their end and halved); the roots flagged, their
//                plus-scan numbers the groups in the order of the root = the smallest locus of each
//   label        per locus its group; loci and bases per group by integer atomics, one per wave and distinct group in the
//                wave.  Sums of integers: the order does not show
//   order        group[q] of the left locus, one stable radix sort of the duplication ordinals by group, group_offsets and
//                the duplications per group by bisection in the sorted keys
#include "tool_base.hpp"

namespace asgart {
namespace {

constexpr uint32_t kBlock = 256;  // threads per workgroup, every kernel; a multiple of the wave size
constexpr uint32_t kGaveUpWalk = 1u, kGaveUpCas = 2u;
constexpr uint32_t kStrides[] = {64, 8, 1};  // the union launches: one duplication in 64, then in 8, then the rest

// (name, end) of a sorted arm: the record of tool_base.hpp's segmented max-scan, which chain.hip shares
using NameEnd = KeyEnd<uint32_t>;

__global__ __launch_bounds__(kBlock) void groups_ends_kernel(const uint32_t *__restrict__ ord,
                                                            const uint32_t *__restrict__ sorted_name,
                                                            const uint64_t *__restrict__ start,
                                                            const uint64_t *__restrict__ length, uint32_t m,
                                                            uint64_t *__restrict__ s_start, NameEnd *__restrict__ pair) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint32_t o = ord[i];
    const uint64_t st = start[o];
    s_start[i] = st;
    pair[i] = NameEnd{st + length[o], sorted_name[i]};  // (the host has refused a sum that wraps)
}

// run[i - 1] is the largest end of all earlier arms of record i's name, where there is one
__global__ __launch_bounds__(kBlock) void groups_heads_kernel(const NameEnd *__restrict__ run,
                                                             const uint64_t *__restrict__ s_start, uint32_t m,
                                                             uint64_t margin, uint32_t *__restrict__ head) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    uint32_t h = 1u;
    if (i > 0) {
        const NameEnd before = run[i - 1];
        h = (before.key != run[i].key || s_start[i] >= sat_add(before.end, margin)) ? 1u : 0u;
    }
    head[i] = h;
}

// every record scatters its locus to its arm; a head opens the locus: name, start, its own slot, and its own parent
__global__ __launch_bounds__(kBlock) void groups_open_kernel(const uint32_t *__restrict__ head,
                                                            const uint32_t *__restrict__ rank,
                                                            const uint32_t *__restrict__ ord, const NameEnd *__restrict__ run,
                                                            const uint64_t *__restrict__ s_start, uint32_t m,
                                                            uint32_t *__restrict__ arm_locus, int32_t *__restrict__ l_name,
                                                            uint64_t *__restrict__ l_start, uint32_t *__restrict__ l_first,
                                                            uint32_t *__restrict__ parent) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint32_t h = head[i], c = rank[i] + h - 1u;  // (rank is exclusive, and record 0 is a head)
    arm_locus[ord[i]] = c;
    if (!h) return;
    l_name[c] = (int32_t)run[i].key;
    l_start[c] = s_start[i];
    l_first[c] = i;
    parent[c] = c;
}

// the last member closes the locus: the running maximum there is its largest end
__global__ __launch_bounds__(kBlock) void groups_close_kernel(const uint32_t *__restrict__ head,
                                                             const uint32_t *__restrict__ rank,
                                                             const NameEnd *__restrict__ run,
                                                             const uint64_t *__restrict__ l_start,
                                                             const uint32_t *__restrict__ l_first, uint32_t m,
                                                             uint64_t *__restrict__ l_length,
                                                             uint32_t *__restrict__ l_members) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || !(i == m - 1 || head[i + 1])) return;
    const uint32_t c = rank[i] + head[i] - 1u;
    l_length[c] = run[i].end - l_start[c];
    l_members[c] = i + 1u - l_first[c];
}

__device__ inline uint32_t parent_of(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path on the way.  parent[y] <= y for every y and a store only lowers it (atomicMin, and only on
// a locus that is no root and never becomes one again), so the walk visits strictly decreasing indices: at most `bound`
// steps.  A walk that is longer sets the give-up bit and answers x itself, which keeps every later index in range.
__device__ inline uint32_t find_root(uint32_t *parent, uint32_t x, uint32_t bound, uint32_t *give_up) {
    const uint32_t from = x;
    for (uint32_t step = 0; step <= bound; ++step) {
        const uint32_t p = parent_of(parent, x);
        if (p == x) return x;
        const uint32_t gp = parent_of(parent, p);
        if (gp == p) return p;  // (p was a root when it was read; not asked again: a group's root is a hot address)
        atomicMin(parent + x, gp);
        x = gp;
    }
    atomicOr(give_up, kGaveUpWalk);
    return from;
}

// Duplication q joins the loci of its two arms.  The larger root goes under the smaller, and only a root is ever hooked
// (the CAS expects parent[hi] == hi).  A CAS that fails has lost to another lane's successful hook of hi; there are fewer
// than `bound` of those in the whole call, so more failures than that set the give-up bit.
// The launches share the work by stride (kStrides: 64, 8, 1): a launch takes the duplications q = t * every that no earlier
// launch took (q % taken != 0).  Between launches groups_compress_kernel points every locus at its root, so that in a
// result with one large group most lanes of the later, larger launches read two parents, find them equal and leave.
__global__ __launch_bounds__(kBlock) void groups_union_kernel(const uint32_t *__restrict__ arm_locus, uint32_t n,
                                                             uint32_t every, uint32_t taken, uint32_t bound,
                                                             uint32_t *parent, uint32_t *give_up) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= (n + every - 1) / every) return;
    const uint32_t q = t * every;  // (below n, which is below 2^31)
    if (taken && q % taken == 0) return;
    uint32_t a = arm_locus[2 * q], b = arm_locus[2 * q + 1];
    // one parent for both: one tree already, whether or not that parent still is a root.  After a compress pass this is how
    // nearly every lane of a large group leaves, without a read of the root's own slot, which every other lane would share
    if (parent_of(parent, a) == parent_of(parent, b)) return;
    for (uint32_t attempt = 0; attempt <= bound; ++attempt) {
        a = find_root(parent, a, bound, give_up);
        b = find_root(parent, b, bound, give_up);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
        a = hi;
        b = lo;
    }
    atomicOr(give_up, kGaveUpCas);
}

// every locus points at its root (nothing is hooked while this runs, so the roots stand still)
__global__ __launch_bounds__(kBlock) void groups_compress_kernel(uint32_t *parent, const uint32_t *__restrict__ total,
                                                                uint32_t bound, uint32_t *give_up) {
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= *total) return;
    const uint32_t r = find_root(parent, x, bound, give_up);
    if (r != x) atomicMin(parent + x, r);
}

// root[x] of every locus, and the root flags with zeros up to slot m: their scan over m + 1 ends in the count of groups
__global__ __launch_bounds__(kBlock) void groups_flatten_kernel(uint32_t *parent, const uint32_t *__restrict__ total,
                                                               uint32_t m, uint32_t *give_up, uint32_t *__restrict__ root,
                                                               uint32_t *__restrict__ is_root) {
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
    if (x > m) return;
    if (x >= *total) {
        is_root[x] = 0u;
        return;
    }
    const uint32_t r = find_root(parent, x, m, give_up);
    root[x] = r;
    is_root[x] = r == x ? 1u : 0u;
}

// per locus its group; per group its loci and their bases, added once per wave and distinct group in the wave (adds to
// one address queue up behind each other, and the usual result has one group that holds nearly every locus)
__global__ __launch_bounds__(kBlock) void groups_label_kernel(const uint32_t *__restrict__ root,
                                                             const uint32_t *__restrict__ g_rank,
                                                             const uint32_t *__restrict__ total,
                                                             const uint64_t *__restrict__ l_length,
                                                             uint32_t *__restrict__ l_group, uint32_t *g_loci,
                                                             unsigned long long *g_bases) {
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = x < *total;
    uint32_t g = 0;
    unsigned long long len = 0;
    if (in_range) {
        g = g_rank[root[x]];
        len = l_length[x];
        l_group[x] = g;
    }
    unsigned long long todo = __ballot(in_range);  // wave-uniform: every lane runs every round, at most 64 of them
    while (todo) {
        const uint32_t g_round = __shfl(g, __ffsll((long long)todo) - 1);
        const bool mine = in_range && g == g_round;
        const unsigned long long same = __ballot(mine);
        unsigned long long sum = mine ? len : 0ull;
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
        if (__lane_id() == 0) {
            atomicAdd(g_loci + g_round, (uint32_t)__popcll(same));
            atomicAdd(g_bases + g_round, sum);
        }
        todo &= ~same;
    }
}

// the sort key of duplication q: the group of its left locus (its right locus has the same)
struct GroupOfDuplication {
    const uint32_t *__restrict__ arm_locus, *__restrict__ l_group;
    __device__ uint32_t operator()(uint32_t q) const { return l_group[arm_locus[2 * q]]; }
};

// group_offsets[g], g in [0, n_groups]: the first sorted duplication whose group is >= g; duplications per group between
__global__ __launch_bounds__(kBlock) void groups_group_offsets_kernel(const uint32_t *__restrict__ sorted_group, uint32_t n,
                                                                     const uint32_t *__restrict__ total,
                                                                     uint64_t *__restrict__ offsets,
                                                                     uint32_t *__restrict__ g_dups) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_groups = *total;
    if (g > n_groups) return;
    const uint32_t at = first_at_least(sorted_group, n, g);
    offsets[g] = at;
    if (g < n_groups) g_dups[g] = first_at_least(sorted_group, n, g + 1u) - at;
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_groups {
    std::vector<uint64_t> name_offsets, l_start, l_length, g_bases, group_offsets;
    std::vector<int32_t> l_name;
    std::vector<uint32_t> l_members, l_group, g_loci, g_dups, group, order, arm_locus;
    double ms[3] = {0, 0, 0};
};

namespace {

const char *const kWho = "asgart_duplication_groups";

struct GroupsWork : ToolWork {
    DevBuf &name = buf(), &start = buf(), &length = buf();
    DevBuf &ord0 = buf(), &key1 = buf(), &ord1 = buf(), &key2 = buf(), &sorted_name = buf(), &ord2 = buf();
    DevBuf &s_start = buf(), &pair = buf(), &run = buf(), &head = buf(), &rank = buf();
    DevBuf &arm_locus = buf(), &l_name = buf(), &l_start = buf(), &l_first = buf(), &l_length = buf(), &l_members = buf();
    DevBuf &name_offsets = buf(), &parent = buf(), &give_up = buf(), &root = buf(), &is_root = buf(), &g_rank = buf();
    DevBuf &l_group = buf(), &g_loci = buf(), &g_bases = buf(), &group = buf(), &dord0 = buf(), &sorted_group = buf();
    DevBuf &order = buf(), &group_offsets = buf(), &g_dups = buf();
};

const char *side_of(int64_t arm) { return (arm & 1) ? "right" : "left"; }

int32_t check_arguments(const int32_t *arm_name, const uint64_t *arm_start, const uint64_t *arm_length, int64_t n_sds,
                        int64_t n_names, asgart_groups **out) {
    if (!out) {
        set_error("%s: bad argument (out is NULL)", kWho);
        return ASGART_E_ARG;
    }
    if (n_sds < 0 || n_names < 0) {
        set_error("%s: a negative count (n_sds = %lld, n_names = %lld)", kWho, (long long)n_sds, (long long)n_names);
        return ASGART_E_ARG;
    }
    if (n_sds > 0 && (!arm_name || !arm_start || !arm_length)) {
        set_error("%s: a NULL arm array with n_sds = %lld", kWho, (long long)n_sds);
        return ASGART_E_ARG;
    }
    if (n_sds >= ((int64_t)1 << 31)) {
        set_error("%s: 2^32 arms and more are not supported", kWho);
        return ASGART_E_CAP;
    }
    for (int64_t j = 0; j < 2 * n_sds; ++j) {
        if (arm_name[j] < 0 || (int64_t)arm_name[j] >= n_names) {
            set_error("%s: arm %lld (duplication %lld, %s) has the name id %d, outside [0, %lld)", kWho, (long long)j,
                      (long long)(j >> 1), side_of(j), (int)arm_name[j], (long long)n_names);
            return ASGART_E_ARG;
        }
        if (arm_length[j] == 0) {
            set_error("%s: arm %lld (duplication %lld, %s) has length 0: an empty arm belongs to no locus", kWho,
                      (long long)j, (long long)(j >> 1), side_of(j));
            return ASGART_E_ARG;
        }
        if (arm_start[j] + arm_length[j] < arm_start[j]) {
            set_error("%s: arm %lld (duplication %lld, %s): start %llu + length %llu wraps past 2^64", kWho, (long long)j,
                      (long long)(j >> 1), side_of(j), (unsigned long long)arm_start[j], (unsigned long long)arm_length[j]);
            return ASGART_E_ARG;
        }
    }
    return 0;
}

int32_t run_groups(GroupsWork &w, asgart_groups *res, const int32_t *arm_name, const uint64_t *arm_start,
                   const uint64_t *arm_length, uint32_t n, uint64_t n_names, uint64_t margin) {
    const uint32_t m = 2 * n;  // arms; no more loci than arms, no more groups than loci
    RC_TRY(w.open(3));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.name, arm_name, (size_t)m * 4));
    RC_TRY(w.upload(w.start, arm_start, (size_t)m * 8));
    RC_TRY(w.upload(w.length, arm_length, (size_t)m * 8));
    for (DevBuf *b : {&w.ord0, &w.ord1, &w.key2, &w.sorted_name, &w.ord2, &w.arm_locus, &w.l_name, &w.l_first, &w.l_members,
                      &w.parent, &w.root, &w.l_group, &w.g_loci, &w.g_dups, &w.group, &w.dord0, &w.sorted_group, &w.order})
        RC_TRY(b->reserve((size_t)m * 4));
    for (DevBuf *b : {&w.key1, &w.s_start, &w.l_start, &w.l_length, &w.g_bases}) RC_TRY(b->reserve((size_t)m * 8));
    for (DevBuf *b : {&w.pair, &w.run}) RC_TRY(b->reserve((size_t)m * sizeof(NameEnd)));
    // one closing zero each: the exclusive scans over m + 1 end in the totals
    for (DevBuf *b : {&w.head, &w.rank, &w.is_root, &w.g_rank}) RC_TRY(b->reserve(((size_t)m + 1) * 4));
    RC_TRY(w.group_offsets.reserve(((size_t)m + 1) * 8));
    RC_TRY(w.name_offsets.reserve((n_names + 1) * 8));
    RC_TRY(w.give_up.reserve(16));
    uint32_t *head = w.head.as<uint32_t>(), *rank = w.rank.as<uint32_t>(), *g_rank = w.g_rank.as<uint32_t>();
    uint32_t *give_up = w.give_up.as<uint32_t>(), *parent = w.parent.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(head + m, 0, 4, s));
    HIP_TRY(hipMemsetAsync(give_up, 0, 4, s));
    HIP_TRY(hipMemsetAsync(w.g_loci.p, 0, (size_t)m * 4, s));
    HIP_TRY(hipMemsetAsync(w.g_bases.p, 0, (size_t)m * 8, s));
    HIP_TRY(hipEventRecord(w.ev[1], s));

    const unsigned grid = blocks_for(m, kBlock), grid1 = blocks_for((uint64_t)m + 1, kBlock);
    // by start (the uploaded column is the key), then by name
    RC_TRY(w.order_pass<uint64_t>(KeyGiven{}, w.start, w.key1, w.ord0, kNoOrder, w.ord1, m, 64));
    RC_TRY(w.order_pass<uint32_t>(ArmName{w.name.as<int32_t>()}, w.key2, w.sorted_name, w.ord1, kOrdered, w.ord2, m,
                                  bits_for(n_names)));
    groups_ends_kernel<<<grid, kBlock, 0, s>>>(w.ord2.as<uint32_t>(), w.sorted_name.as<uint32_t>(), w.start.as<uint64_t>(),
                                               w.length.as<uint64_t>(), m, w.s_start.as<uint64_t>(), w.pair.as<NameEnd>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.segmented_max_scan(w.pair.as<NameEnd>(), w.run.as<NameEnd>(), m));
    groups_heads_kernel<<<grid, kBlock, 0, s>>>(w.run.as<NameEnd>(), w.s_start.as<uint64_t>(), m, margin, head);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(head, rank, (size_t)m + 1));
    groups_open_kernel<<<grid, kBlock, 0, s>>>(head, rank, w.ord2.as<uint32_t>(), w.run.as<NameEnd>(),
                                               w.s_start.as<uint64_t>(), m, w.arm_locus.as<uint32_t>(),
                                               w.l_name.as<int32_t>(), w.l_start.as<uint64_t>(), w.l_first.as<uint32_t>(),
                                               parent);
    HIP_TRY(hipGetLastError());
    groups_close_kernel<<<grid, kBlock, 0, s>>>(head, rank, w.run.as<NameEnd>(), w.l_start.as<uint64_t>(),
                                                w.l_first.as<uint32_t>(), m, w.l_length.as<uint64_t>(),
                                                w.l_members.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    // row k of the name offsets: the first locus whose name is >= k; the count of loci is the scan's total
    row_offsets_kernel<kBlock><<<blocks_for(n_names + 1, kBlock), kBlock, 0, s>>>(w.l_name.as<int32_t>(), rank + m, n_names,
                                                                                  w.name_offsets.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    uint32_t taken = 0;
    for (uint32_t every : kStrides) {
        if (taken) {
            groups_compress_kernel<<<grid, kBlock, 0, s>>>(parent, rank + m, m, give_up);
            HIP_TRY(hipGetLastError());
        }
        groups_union_kernel<<<blocks_for((n + every - 1) / every, kBlock), kBlock, 0, s>>>(w.arm_locus.as<uint32_t>(), n, every,
                                                                                       taken, m, parent, give_up);
        HIP_TRY(hipGetLastError());
        taken = every;
    }
    groups_flatten_kernel<<<grid1, kBlock, 0, s>>>(parent, rank + m, m, give_up, w.root.as<uint32_t>(),
                                                   w.is_root.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.is_root.as<uint32_t>(), g_rank, (size_t)m + 1));
    groups_label_kernel<<<grid, kBlock, 0, s>>>(w.root.as<uint32_t>(), g_rank, rank + m, w.l_length.as<uint64_t>(),
                                                w.l_group.as<uint32_t>(), w.g_loci.as<uint32_t>(),
                                                w.g_bases.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    // the duplications by group: an ordering of its own, one pass
    RC_TRY(w.order_pass<uint32_t>(GroupOfDuplication{w.arm_locus.as<uint32_t>(), w.l_group.as<uint32_t>()}, w.group,
                                  w.sorted_group, w.dord0, kNoOrder, w.order, n, bits_for(m)));
    groups_group_offsets_kernel<<<grid1, kBlock, 0, s>>>(w.sorted_group.as<uint32_t>(), n, g_rank + m,
                                                         w.group_offsets.as<uint64_t>(), w.g_dups.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[2], s));

    uint32_t n_loci = 0, n_groups = 0, gave_up = 0;  // the counts that size the output, and whether a bound was met
    HIP_TRY(read_back(&n_loci, rank + m, 4, s));
    HIP_TRY(read_back(&n_groups, g_rank + m, 4, s));
    HIP_TRY(read_back(&gave_up, give_up, 4, s));
    if (gave_up) {
        set_error("%s: the union-find gave up (%s%s): more than %u steps where the rule allows no more", kWho,
                  (gave_up & kGaveUpWalk) ? "a parent walk" : "", (gave_up & kGaveUpCas) ? " a hook's retries" : "", m);
        return ASGART_E_HIP;
    }
    if (n_loci == 0 || n_loci > m || n_groups == 0 || n_groups > n_loci) {
        set_error("%s: %u loci and %u groups of %u arms", kWho, n_loci, n_groups, m);
        return ASGART_E_HIP;
    }
    w.start_copy_back();
    RC_TRY(w.fetch(res->name_offsets, w.name_offsets, n_names + 1));
    RC_TRY(w.fetch(res->l_name, w.l_name, n_loci));
    RC_TRY(w.fetch(res->l_start, w.l_start, n_loci));
    RC_TRY(w.fetch(res->l_length, w.l_length, n_loci));
    RC_TRY(w.fetch(res->l_members, w.l_members, n_loci));
    RC_TRY(w.fetch(res->l_group, w.l_group, n_loci));
    RC_TRY(w.fetch(res->g_loci, w.g_loci, n_groups));
    RC_TRY(w.fetch(res->g_dups, w.g_dups, n_groups));
    RC_TRY(w.fetch(res->g_bases, w.g_bases, n_groups));
    RC_TRY(w.fetch(res->group, w.group, n));
    RC_TRY(w.fetch(res->order, w.order, n));
    RC_TRY(w.fetch(res->group_offsets, w.group_offsets, (size_t)n_groups + 1));
    RC_TRY(w.fetch(res->arm_locus, w.arm_locus, m));
    HIP_TRY(stream_sync(s));
    return w.figures(res->ms);
}

}  // namespace

extern "C" int32_t asgart_duplication_groups(int32_t device, const int32_t *arm_name, const uint64_t *arm_start,
                                             const uint64_t *arm_length, int64_t n_sds, int64_t n_names, uint64_t margin,
                                             asgart_groups **out) {
    if (out) *out = nullptr;
    RC_TRY(check_arguments(arm_name, arm_start, arm_length, n_sds, n_names, out));
    RC_TRY(use_device(kWho, device));
    if (n_sds == 0) {  // empty rows, no groups; nothing is launched
        *out = new asgart_groups;
        (*out)->name_offsets.assign((size_t)n_names + 1, 0);
        (*out)->group_offsets.assign(1, 0);
        return 0;
    }
    return run_tool<GroupsWork>(out, [&](GroupsWork &w, asgart_groups *res) {
        return run_groups(w, res, arm_name, arm_start, arm_length, (uint32_t)n_sds, (uint64_t)n_names, margin);
    });
}

extern "C" void asgart_groups_counts(const asgart_groups *r, uint64_t *n_names, uint64_t *n_loci, uint64_t *n_groups) {
    if (n_names) *n_names = r ? r->name_offsets.size() - 1 : 0;
    if (n_loci) *n_loci = r ? r->l_start.size() : 0;
    if (n_groups) *n_groups = r ? r->g_loci.size() : 0;
}

extern "C" void asgart_groups_copy(const asgart_groups *r, uint64_t *name_offsets, int32_t *locus_name,
                                   uint64_t *locus_start, uint64_t *locus_length, uint32_t *locus_members,
                                   uint32_t *locus_group, uint32_t *group_loci, uint32_t *group_duplications,
                                   uint64_t *group_bases, uint32_t *group, uint32_t *order, uint64_t *group_offsets,
                                   uint32_t *arm_locus) {
    if (!r) return;
    give(name_offsets, r->name_offsets);
    give(locus_name, r->l_name);
    give(locus_start, r->l_start);
    give(locus_length, r->l_length);
    give(locus_members, r->l_members);
    give(locus_group, r->l_group);
    give(group_loci, r->g_loci);
    give(group_duplications, r->g_dups);
    give(group_bases, r->g_bases);
    give(group, r->group);
    give(order, r->order);
    give(group_offsets, r->group_offsets);
    give(arm_locus, r->arm_locus);
}

extern "C" int32_t asgart_groups_timings(const asgart_groups *r, double *ms3) {
    return copy_ms3("asgart_groups_timings", r, ms3);
}

extern "C" void asgart_groups_free(asgart_groups *r) { delete r; }

extern "C" void asgart_groups_geometry(uint64_t *block_threads) {
    if (block_threads) *block_threads = kBlock;
}
