// rosary.hip -- the duplicon clusters of the rosary plot for every fragment name at once: asgart_rosary_clusters and its
// handle.
//
// Replaces RosaryPlotter::duplicons_for_chr, reference src/plot/rosary_plot.rs:123-192, which for every fragment of the map
// walks every duplication of the result, compares names as strings, sorts that fragment's arms by start (stable) and folds
// them into clusters one by one: `new` joins `last` when new.start <= last.start + last.length + margin (:164), and then
// last.length = new.start + new.length - last.start (:165).  After every iteration last.start + last.length is the END OF
// THE SPAN JUST HANDLED (after a push `last` is the span itself), so whether span i opens a cluster depends on span i - 1
// alone:
//
//   head[i] = i == 0 || name[i] != name[i - 1] || start[i] > end[i - 1] + margin        (u64, every + wrapping)
//
// in the order of a stable sort by (name, start) of the arms in flatten order (duplication q, left then right: ordinal
// 2q + side).  A cluster starts where its head starts, ends where its LAST member ends (not at the largest end: a contained
// short span shortens it), has its head's (reversed, complemented) and `both` when a member's differ from the head's (:178).
//
// Stages, all on one stream, nothing read back but the cluster count at the very end:
//   emit      the ordinals 0 .. 2n - 1 (the sort's values; start, end and the flag bits are gathered by ordinal afterwards,
//             which moves 4 bytes per record through the sorts instead of 21)
//   sort      radix sort on the 64-bit start carrying the ordinal, then a stable radix sort on the name bits only: ties keep
//             flatten order, which decides the head and with it the colour
//   heads     one thread per sorted record: gathers start, end = start + length and the two flag bits; the previous
//             record's name and end come from the neighbour lane (__shfl_up), the wave's first lane loads them
//   scan      exclusive scan of the head flags (one closing zero): cluster ordinal per record, cluster count at the end
//   reduce    a head writes name, start and flag bits; then the last member writes end - start[head], and `both` / `members`
//             are combined per wave first (a cluster is a run of consecutive records: ballots over the run) and added with
//             at most one atomic per cluster per wave, none for `both` when no lane of the run differs from the head.  A
//             cluster may span any number of workgroups.
//   offsets   row k of the name offsets = the first cluster whose name is >= k (bisection in the clusters' names)
#include "tool_base.hpp"

namespace asgart {
namespace {

constexpr uint32_t kBlock = 256;  // threads per workgroup, every kernel; a multiple of the wave size

// sorted record i: start, end, flag bits; head[i] by the predicate on record i - 1.  Every lane runs the shuffles.
__global__ __launch_bounds__(kBlock) void rosary_heads_kernel(const uint32_t *__restrict__ ord,
                                                             const uint32_t *__restrict__ sorted_name,
                                                             const uint64_t *__restrict__ start,
                                                             const uint64_t *__restrict__ length,
                                                             const uint8_t *__restrict__ flags, uint32_t m, uint64_t margin,
                                                             uint64_t *__restrict__ s_start, uint64_t *__restrict__ s_end,
                                                             uint8_t *__restrict__ s_bits, uint32_t *__restrict__ head) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < m;
    uint32_t nm = 0, o = 0;
    uint64_t st = 0, en = 0;
    if (in_range) {
        o = ord[i];
        nm = sorted_name[i];
        st = start[o];
        en = st + length[o];
    }
    uint32_t pn = __shfl_up(nm, 1);
    uint64_t pe = (uint64_t)__shfl_up((unsigned long long)en, 1);
    if (!in_range) return;
    if (__lane_id() == 0 && i > 0) {
        const uint32_t po = ord[i - 1];
        pn = sorted_name[i - 1];
        pe = start[po] + length[po];
    }
    s_start[i] = st;
    s_end[i] = en;
    s_bits[i] = flags ? (uint8_t)(flags[o >> 1] & 3u) : (uint8_t)0;
    head[i] = (i == 0 || nm != pn || st > pe + margin) ? 1u : 0u;
}

// a head opens its cluster: name, start, the class bits of the first member, no members yet
__global__ __launch_bounds__(kBlock) void rosary_open_kernel(const uint32_t *__restrict__ head,
                                                            const uint32_t *__restrict__ rank,
                                                            const uint32_t *__restrict__ sorted_name,
                                                            const uint64_t *__restrict__ s_start,
                                                            const uint8_t *__restrict__ s_bits, uint32_t m,
                                                            uint32_t *__restrict__ c_name, uint64_t *__restrict__ c_start,
                                                            uint32_t *__restrict__ c_klass, uint32_t *__restrict__ c_members) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || !head[i]) return;
    const uint32_t c = rank[i];
    c_name[c] = sorted_name[i];
    c_start[c] = s_start[i];
    c_klass[c] = s_bits[i];
    c_members[c] = 0u;
}

// every record joins its cluster.  Within a wave the records of one cluster are a run of lanes that begins at lane 0 or at
// a head: the run's first lane counts the run and asks whether any of it differs from the head -- one atomicAdd, and one
// atomicOr only where something differs.  The cluster's last record writes the length.
__global__ __launch_bounds__(kBlock) void rosary_join_kernel(const uint32_t *__restrict__ head,
                                                            const uint32_t *__restrict__ rank,
                                                            const uint64_t *__restrict__ s_end,
                                                            const uint8_t *__restrict__ s_bits, uint32_t m,
                                                            const uint64_t *__restrict__ c_start,
                                                            uint64_t *__restrict__ c_length, uint32_t *c_klass,
                                                            uint32_t *c_members) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = __lane_id();
    const bool in_range = i < m;
    const uint32_t h = in_range ? head[i] : 0u;
    const uint32_t c = in_range ? rank[i] + h - 1u : 0u;
    // (bits 0 and 1 of c_klass were written by rosary_open_kernel and do not change here)
    const bool differs = in_range && (uint32_t)s_bits[i] != (c_klass[c] & 3u);
    const bool opens = in_range && (lane == 0 || h);
    const unsigned long long in_mask = __ballot(in_range), open_mask = __ballot(opens), diff_mask = __ballot(differs);
    if (opens) {
        const unsigned long long above = lane == 63 ? 0ull : open_mask & (~0ull << (lane + 1));
        const int end_lane = above ? __ffsll((long long)above) - 1 : 64;  // the run is [lane, end_lane)
        const unsigned long long run = (end_lane == 64 ? ~0ull : (1ull << end_lane) - 1ull) & (~0ull << lane) & in_mask;
        atomicAdd(c_members + c, (uint32_t)__popcll(run));
        if (diff_mask & run) atomicOr(c_klass + c, 4u);
    }
    if (in_range && (i == m - 1 || head[i + 1])) c_length[c] = s_end[i] - c_start[c];
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_rosary {
    std::vector<uint64_t> offsets, start, length;
    std::vector<uint8_t> klass;
    std::vector<uint32_t> members;
    double ms[3] = {0, 0, 0};
};

namespace {

struct RosaryWork : ToolWork {
    DevBuf &name = buf(), &start = buf(), &length = buf(), &flags = buf();
    DevBuf &ord0 = buf(), &key1 = buf(), &ord1 = buf(), &key2 = buf(), &sorted_name = buf(), &ord2 = buf();
    DevBuf &s_start = buf(), &s_end = buf(), &s_bits = buf(), &head = buf(), &rank = buf();
    DevBuf &c_name = buf(), &c_start = buf(), &c_length = buf(), &c_klass = buf(), &c_members = buf(), &offsets = buf();
};

int32_t check_arguments(const int32_t *arm_name, const uint64_t *arm_start, const uint64_t *arm_length, int64_t n_sds,
                        int64_t n_names, asgart_rosary **out) {
    if (!out || n_sds < 0 || n_names < 0 || (n_sds > 0 && (!arm_name || !arm_start || !arm_length))) {
        set_error("asgart_rosary_clusters: bad argument");
        return ASGART_E_ARG;
    }
    if (n_sds >= ((int64_t)1 << 31)) {
        set_error("asgart_rosary_clusters: 2^32 arms and more are not supported");
        return ASGART_E_CAP;
    }
    for (int64_t j = 0; j < 2 * n_sds; ++j)
        if (arm_name[j] < 0 || (int64_t)arm_name[j] >= n_names) {
            set_error("asgart_rosary_clusters: arm %lld (duplication %lld, %s) has the name id %d, outside [0, %lld)",
                      (long long)j, (long long)(j >> 1), (j & 1) ? "right" : "left", (int)arm_name[j], (long long)n_names);
            return ASGART_E_ARG;
        }
    return 0;
}

int32_t run_rosary(RosaryWork &w, asgart_rosary *res, const int32_t *arm_name, const uint64_t *arm_start,
                   const uint64_t *arm_length, const uint8_t *flags, uint32_t n, uint64_t n_names, uint64_t margin) {
    const uint32_t m = 2 * n;  // arms
    RC_TRY(w.open(3));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.name, arm_name, (size_t)m * 4));
    RC_TRY(w.upload(w.start, arm_start, (size_t)m * 8));
    RC_TRY(w.upload(w.length, arm_length, (size_t)m * 8));
    if (flags) RC_TRY(w.upload(w.flags, flags, n));
    for (DevBuf *b : {&w.ord0, &w.ord1, &w.key2, &w.sorted_name, &w.ord2, &w.c_name, &w.c_klass, &w.c_members})
        RC_TRY(b->reserve((size_t)m * 4));
    for (DevBuf *b : {&w.key1, &w.s_start, &w.s_end, &w.c_start, &w.c_length}) RC_TRY(b->reserve((size_t)m * 8));
    RC_TRY(w.s_bits.reserve((size_t)m + 16));
    RC_TRY(w.head.reserve(((size_t)m + 1) * 4));  // one closing zero: the exclusive scan over m + 1 ends in the total
    RC_TRY(w.rank.reserve(((size_t)m + 1) * 4));
    RC_TRY(w.offsets.reserve((n_names + 1) * 8));
    uint32_t *head = w.head.as<uint32_t>(), *rank = w.rank.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(head + m, 0, 4, s));
    HIP_TRY(hipEventRecord(w.ev[1], s));

    const unsigned grid = blocks_for(m);
    // by start (the uploaded column is the key), then by name
    RC_TRY(w.order_pass<uint64_t>(KeyGiven{}, w.start, w.key1, w.ord0, kNoOrder, w.ord1, m, 64));
    RC_TRY(w.order_pass<uint32_t>(ArmName{w.name.as<int32_t>()}, w.key2, w.sorted_name, w.ord1, kOrdered, w.ord2, m,
                                  bits_for(n_names)));
    rosary_heads_kernel<<<grid, kBlock, 0, s>>>(w.ord2.as<uint32_t>(), w.sorted_name.as<uint32_t>(), w.start.as<uint64_t>(),
                                                w.length.as<uint64_t>(), flags ? w.flags.as<uint8_t>() : nullptr, m, margin,
                                                w.s_start.as<uint64_t>(), w.s_end.as<uint64_t>(), w.s_bits.as<uint8_t>(), head);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(head, rank, (size_t)m + 1));
    rosary_open_kernel<<<grid, kBlock, 0, s>>>(head, rank, w.sorted_name.as<uint32_t>(), w.s_start.as<uint64_t>(),
                                               w.s_bits.as<uint8_t>(), m, w.c_name.as<uint32_t>(), w.c_start.as<uint64_t>(),
                                               w.c_klass.as<uint32_t>(), w.c_members.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    rosary_join_kernel<<<grid, kBlock, 0, s>>>(head, rank, w.s_end.as<uint64_t>(), w.s_bits.as<uint8_t>(), m,
                                               w.c_start.as<uint64_t>(), w.c_length.as<uint64_t>(), w.c_klass.as<uint32_t>(),
                                               w.c_members.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    // row k of the name offsets: the first cluster whose name is >= k; the count of clusters is the scan's total
    row_offsets_kernel<kBlock><<<blocks_for(n_names + 1, kBlock), kBlock, 0, s>>>(w.c_name.as<uint32_t>(), rank + m, n_names,
                                                                                  w.offsets.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[2], s));

    uint32_t nc = 0;  // the one count that sizes the output
    HIP_TRY(read_back(&nc, rank + m, 4, s));
    if (nc == 0 || nc > m) {
        set_error("asgart_rosary_clusters: %u clusters of %u arms", nc, m);
        return ASGART_E_HIP;
    }
    w.start_copy_back();
    std::vector<uint32_t> klass32;
    RC_TRY(w.fetch(res->offsets, w.offsets, n_names + 1));
    RC_TRY(w.fetch(res->start, w.c_start, nc));
    RC_TRY(w.fetch(res->length, w.c_length, nc));
    RC_TRY(w.fetch(res->members, w.c_members, nc));
    RC_TRY(w.fetch(klass32, w.c_klass, nc));
    HIP_TRY(stream_sync(s));
    res->klass.assign(klass32.begin(), klass32.end());  // (words on the device, where atomicOr sets `both`; bytes in the handle)
    return w.figures(res->ms);
}

}  // namespace

extern "C" int32_t asgart_rosary_clusters(int32_t device, const int32_t *arm_name, const uint64_t *arm_start,
                                          const uint64_t *arm_length, const uint8_t *flags, int64_t n_sds, int64_t n_names,
                                          uint64_t margin, asgart_rosary **out) {
    if (out) *out = nullptr;
    RC_TRY(check_arguments(arm_name, arm_start, arm_length, n_sds, n_names, out));
    RC_TRY(use_device("asgart_rosary_clusters", device));
    if (n_sds == 0) {  // empty rows; nothing is launched
        *out = new asgart_rosary;
        (*out)->offsets.assign((size_t)n_names + 1, 0);
        return 0;
    }
    return run_tool<RosaryWork>(out, [&](RosaryWork &w, asgart_rosary *res) {
        return run_rosary(w, res, arm_name, arm_start, arm_length, flags, (uint32_t)n_sds, (uint64_t)n_names, margin);
    });
}

extern "C" void asgart_rosary_counts(const asgart_rosary *r, uint64_t *n_names, uint64_t *n_clusters) {
    if (n_names) *n_names = r ? r->offsets.size() - 1 : 0;
    if (n_clusters) *n_clusters = r ? r->start.size() : 0;
}

extern "C" void asgart_rosary_copy(const asgart_rosary *r, uint64_t *name_offsets, uint64_t *start, uint64_t *length,
                                   uint8_t *klass, uint32_t *members) {
    if (!r) return;
    give(name_offsets, r->offsets);
    give(start, r->start);
    give(length, r->length);
    give(klass, r->klass);
    give(members, r->members);
}

extern "C" int32_t asgart_rosary_timings(const asgart_rosary *r, double *ms3) {
    return copy_ms3("asgart_rosary_timings", r, ms3);
}

extern "C" void asgart_rosary_free(asgart_rosary *r) { delete r; }

extern "C" void asgart_rosary_geometry(uint64_t *block_threads) {
    if (block_threads) *block_threads = kBlock;
}
