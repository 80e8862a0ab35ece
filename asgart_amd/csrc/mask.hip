// mask.hip -- which bases of the strand the arms of a result cover: asgart_mask_intervals and its handle.  The rule is stated
// once, in include/asgart_hip.h; asgart_amd/mask.py: intervals_host is the readable statement of it.
//
// groups.hip next door folds the arms into loci PER NAME and never counts how many arms lie on a base; here the arms are laid
// on the strand (a record's start added, the margin clipped at the record's two ends) and a base counts when at least
// min_depth arms hold it: a coverage sweep.  What is shared is tool_base.hpp.
//
// Stages, all on one stream; three words are read back at the very end, then the pairs:
//   events       one thread per arm: (clipped start, +1) and (clipped end, -1), strand coordinates
//   sort         the events by their 64-bit position (rocPRIM radix sort, the delta goes with its key)
//   depth        exclusive plus-scan of the deltas; depth[i] + delta[i] at the LAST event of a position is the depth behind
//                that position -- the deltas of equal positions are summed by the scan itself, in whatever order the sort left
//                them, so [0,10) and [10,20) meet in one position whose sum is 0
//   positions    the last event of every position is flagged; the plus-scan of the flags numbers the distinct positions,
//                and each writes (position, depth behind it) to its slot; the largest depth goes through one atomic maximum
//                per wave
//   edges        position k is an edge iff (depth behind k - 1 >= D) != (depth behind k >= D); the plus-scan of the edges
//                places them: edge 2i opens interval i, edge 2i + 1 closes it (the depth ends at 0, so they pair up), and
//                the masked bases are the sum of the closing minus the opening positions: one 64-bit atomic add per wave,
//                a sum of integers modulo 2^64, so the order does not show
// No thread walks an arm or an interval, everything is integer, and nothing depends on the order of arrival.
#include "tool_base.hpp"

namespace asgart {
namespace {

constexpr uint32_t kBlock = 256;  // threads per workgroup, every kernel; a multiple of the wave size

__host__ __device__ inline uint64_t sat_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~(uint64_t)0 : s;
}

// (the host has checked: the record id is in the table, length >= 1, start + length <= record_len)
__global__ __launch_bounds__(kBlock) void mask_events_kernel(const int32_t *__restrict__ arm_record,
                                                            const uint64_t *__restrict__ arm_start,
                                                            const uint64_t *__restrict__ arm_length,
                                                            const uint64_t *__restrict__ record_start,
                                                            const uint64_t *__restrict__ record_len, uint32_t n_arms,
                                                            uint64_t margin, uint64_t *__restrict__ pos,
                                                            uint32_t *__restrict__ delta) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_arms) return;
    const uint32_t r = (uint32_t)arm_record[j];
    const uint64_t rs = record_start[r], st = arm_start[j];
    const uint64_t lo = st > margin ? st - margin : 0;
    const uint64_t hi = min(record_len[r], sat_add(st + arm_length[j], margin));
    pos[2 * (size_t)j] = rs + lo;
    delta[2 * (size_t)j] = 1u;
    pos[2 * (size_t)j + 1] = rs + hi;
    delta[2 * (size_t)j + 1] = ~0u;   // -1: the depths are sums modulo 2^32 of fewer than 2^31 arms
}

// last[i] = event i is the last of its position; slot m (the closing entry of the scan) is 0
__global__ __launch_bounds__(kBlock) void mask_last_kernel(const uint64_t *__restrict__ pos, uint32_t m,
                                                          uint32_t *__restrict__ last) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > m) return;
    last[i] = (i < m && (i + 1 == m || pos[i + 1] != pos[i])) ? 1u : 0u;
}

__device__ inline uint32_t wave_max(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_down(v, d));
    return v;
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// the last event of a position writes the position and the depth behind it to the position's slot
__global__ __launch_bounds__(kBlock) void mask_positions_kernel(const uint64_t *__restrict__ pos,
                                                               const uint32_t *__restrict__ delta,
                                                               const uint32_t *__restrict__ before,
                                                               const uint32_t *__restrict__ last,
                                                               const uint32_t *__restrict__ slot, uint32_t m,
                                                               uint64_t *__restrict__ u_pos, uint32_t *__restrict__ u_depth,
                                                               uint32_t *max_depth) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t depth = 0;
    if (i < m && last[i]) {
        depth = before[i] + delta[i];
        u_pos[slot[i]] = pos[i];
        u_depth[slot[i]] = depth;
    }
    depth = wave_max(depth);   // (every lane of the wave is here: no lane has returned)
    if (__lane_id() == 0 && depth) atomicMax(max_depth, depth);
}

// edge[k] = the test depth >= D changes at position k; slot *n_pos and every slot behind it is 0
__global__ __launch_bounds__(kBlock) void mask_edges_kernel(const uint32_t *__restrict__ u_depth,
                                                           const uint32_t *__restrict__ n_pos, uint32_t m, uint32_t min_depth,
                                                           uint32_t *__restrict__ edge) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k > m) return;
    uint32_t e = 0;
    if (k < *n_pos) {
        const bool was = k > 0 && u_depth[k - 1] >= min_depth, is = u_depth[k] >= min_depth;
        e = was != is ? 1u : 0u;
    }
    edge[k] = e;
}

// edge number r is bound r of the pairs: even ones open an interval, odd ones close it
__global__ __launch_bounds__(kBlock) void mask_pairs_kernel(const uint64_t *__restrict__ u_pos,
                                                           const uint32_t *__restrict__ edge,
                                                           const uint32_t *__restrict__ rank, uint32_t m,
                                                           uint64_t *__restrict__ bounds, unsigned long long *masked) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long part = 0;
    if (k < m && edge[k]) {
        const uint32_t r = rank[k];
        const uint64_t p = u_pos[k];
        bounds[r] = p;
        part = (r & 1u) ? p : (unsigned long long)0 - p;
    }
    part = wave_sum(part);
    if (__lane_id() == 0 && part) atomicAdd(masked, part);
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_mask {
    std::vector<uint64_t> bounds;  // (start, end) pairs
    uint64_t masked = 0, max_depth = 0;
    double ms[3] = {0, 0, 0};
};

namespace {

const char *const kWho = "asgart_mask_intervals";

struct MaskWork : ToolWork {
    DevBuf &arm_record = buf(), &arm_start = buf(), &arm_length = buf(), &record_start = buf(), &record_len = buf();
    DevBuf &pos0 = buf(), &delta0 = buf(), &pos = buf(), &delta = buf(), &before = buf(), &last = buf(), &slot = buf();
    DevBuf &u_pos = buf(), &u_depth = buf(), &edge = buf(), &rank = buf(), &bounds = buf(), &words = buf();
};

int32_t check_arguments(const int32_t *arm_record, const uint64_t *arm_start, const uint64_t *arm_length, int64_t n_arms,
                        const uint64_t *record_start, const uint64_t *record_len, int64_t n_records, uint32_t min_depth,
                        asgart_mask **out) {
    if (!out) {
        set_error("%s: bad argument (out is NULL)", kWho);
        return ASGART_E_ARG;
    }
    if (n_arms < 0 || n_records < 0) {
        set_error("%s: a negative count (n_arms = %lld, n_records = %lld)", kWho, (long long)n_arms, (long long)n_records);
        return ASGART_E_ARG;
    }
    if (n_arms > 0 && (!arm_record || !arm_start || !arm_length)) {
        set_error("%s: a NULL arm array with n_arms = %lld", kWho, (long long)n_arms);
        return ASGART_E_ARG;
    }
    if (n_records > 0 && (!record_start || !record_len)) {
        set_error("%s: a NULL record array with n_records = %lld", kWho, (long long)n_records);
        return ASGART_E_ARG;
    }
    if (min_depth == 0) {
        set_error("%s: min_depth is 0: every base of the strand has depth >= 0 (1 masks what any arm covers)", kWho);
        return ASGART_E_ARG;
    }
    if (n_arms >= ((int64_t)1 << 31)) {
        set_error("%s: 2^31 arms and more are not supported", kWho);
        return ASGART_E_CAP;
    }
    for (int64_t r = 0; r < n_records; ++r) {
        const uint64_t end = record_start[r] + record_len[r];
        if (end < record_start[r] || (r + 1 < n_records && end > record_start[r + 1])) {
            set_error("%s: record %lld (start %llu, length %llu) wraps or reaches into the next: the records must be "
                      "ascending and must not overlap", kWho, (long long)r, (unsigned long long)record_start[r],
                      (unsigned long long)record_len[r]);
            return ASGART_E_ARG;
        }
    }
    for (int64_t j = 0; j < n_arms; ++j) {
        if (arm_record[j] < 0 || (int64_t)arm_record[j] >= n_records) {
            set_error("%s: arm %lld has the record id %d, outside [0, %lld)", kWho, (long long)j, (int)arm_record[j],
                      (long long)n_records);
            return ASGART_E_ARG;
        }
        if (arm_length[j] == 0) {
            set_error("%s: arm %lld has length 0: an empty arm covers no base", kWho, (long long)j);
            return ASGART_E_ARG;
        }
        const uint64_t len = record_len[arm_record[j]];
        if (arm_start[j] > len || arm_length[j] > len - arm_start[j]) {
            set_error("%s: arm %lld: start %llu + length %llu leaves its record %d of %llu bases: the result does not "
                      "belong to these records", kWho, (long long)j, (unsigned long long)arm_start[j],
                      (unsigned long long)arm_length[j], (int)arm_record[j], (unsigned long long)len);
            return ASGART_E_ARG;
        }
    }
    return 0;
}

int32_t run_mask(MaskWork &w, asgart_mask *res, const int32_t *arm_record, const uint64_t *arm_start,
                 const uint64_t *arm_length, uint32_t n_arms, const uint64_t *record_start, const uint64_t *record_len,
                 size_t n_records, uint64_t margin, uint32_t min_depth) {
    const uint32_t m = 2 * n_arms;  // events; no more positions than events, no more edges than positions
    RC_TRY(w.open(3));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.arm_record, arm_record, (size_t)n_arms * 4));
    RC_TRY(w.upload(w.arm_start, arm_start, (size_t)n_arms * 8));
    RC_TRY(w.upload(w.arm_length, arm_length, (size_t)n_arms * 8));
    RC_TRY(w.upload(w.record_start, record_start, n_records * 8));
    RC_TRY(w.upload(w.record_len, record_len, n_records * 8));
    for (DevBuf *b : {&w.pos0, &w.pos, &w.u_pos, &w.bounds}) RC_TRY(b->reserve((size_t)m * 8));
    for (DevBuf *b : {&w.delta0, &w.delta, &w.before, &w.u_depth}) RC_TRY(b->reserve((size_t)m * 4));
    // one closing zero each: the exclusive scans over m + 1 end in the totals
    for (DevBuf *b : {&w.last, &w.slot, &w.edge, &w.rank}) RC_TRY(b->reserve(((size_t)m + 1) * 4));
    RC_TRY(w.words.reserve(16));  // [0, 8): the masked bases, [8, 12): the largest depth
    HIP_TRY(hipMemsetAsync(w.words.p, 0, 16, s));
    HIP_TRY(hipEventRecord(w.ev[1], s));

    uint32_t *slot = w.slot.as<uint32_t>(), *rank = w.rank.as<uint32_t>();
    unsigned long long *masked = w.words.as<unsigned long long>();
    uint32_t *max_depth = w.words.as<uint32_t>() + 2;
    const unsigned grid = blocks_for(m, kBlock), grid1 = blocks_for((uint64_t)m + 1, kBlock);
    mask_events_kernel<<<blocks_for(n_arms, kBlock), kBlock, 0, s>>>(
        w.arm_record.as<int32_t>(), w.arm_start.as<uint64_t>(), w.arm_length.as<uint64_t>(), w.record_start.as<uint64_t>(),
        w.record_len.as<uint64_t>(), n_arms, margin, w.pos0.as<uint64_t>(), w.delta0.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.sort_pairs(w.pos0.as<uint64_t>(), w.pos.as<uint64_t>(), w.delta0.as<uint32_t>(), w.delta.as<uint32_t>(), m, 64));
    RC_TRY(w.exclusive_scan(w.delta.as<uint32_t>(), w.before.as<uint32_t>(), (size_t)m));
    mask_last_kernel<<<grid1, kBlock, 0, s>>>(w.pos.as<uint64_t>(), m, w.last.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.last.as<uint32_t>(), slot, (size_t)m + 1));
    mask_positions_kernel<<<grid, kBlock, 0, s>>>(w.pos.as<uint64_t>(), w.delta.as<uint32_t>(), w.before.as<uint32_t>(),
                                                  w.last.as<uint32_t>(), slot, m, w.u_pos.as<uint64_t>(),
                                                  w.u_depth.as<uint32_t>(), max_depth);
    HIP_TRY(hipGetLastError());
    mask_edges_kernel<<<grid1, kBlock, 0, s>>>(w.u_depth.as<uint32_t>(), slot + m, m, min_depth, w.edge.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.edge.as<uint32_t>(), rank, (size_t)m + 1));
    mask_pairs_kernel<<<grid, kBlock, 0, s>>>(w.u_pos.as<uint64_t>(), w.edge.as<uint32_t>(), rank, m,
                                              w.bounds.as<uint64_t>(), masked);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[2], s));

    uint32_t n_edges = 0;
    uint64_t words[2] = {0, 0};
    HIP_TRY(read_back(&n_edges, rank + m, 4, s));
    HIP_TRY(read_back(words, w.words.p, 16, s));
    if (n_edges > m || (n_edges & 1u)) {
        set_error("%s: %u interval bounds of %u events", kWho, n_edges, m);
        return ASGART_E_HIP;
    }
    res->masked = words[0];
    res->max_depth = (uint32_t)words[1];
    w.start_copy_back();
    RC_TRY(w.fetch(res->bounds, w.bounds, n_edges));
    HIP_TRY(stream_sync(s));
    return w.figures(res->ms);
}

}  // namespace

extern "C" int32_t asgart_mask_intervals(int32_t device, const int32_t *arm_record, const uint64_t *arm_start,
                                         const uint64_t *arm_length, int64_t n_arms, const uint64_t *record_start,
                                         const uint64_t *record_len, int64_t n_records, uint64_t margin, uint32_t min_depth,
                                         asgart_mask **out) {
    if (out) *out = nullptr;
    RC_TRY(check_arguments(arm_record, arm_start, arm_length, n_arms, record_start, record_len, n_records, min_depth, out));
    RC_TRY(use_device(kWho, device));
    if (n_arms == 0) {  // no intervals; nothing is launched
        *out = new asgart_mask;
        return 0;
    }
    return run_tool<MaskWork>(out, [&](MaskWork &w, asgart_mask *res) {
        return run_mask(w, res, arm_record, arm_start, arm_length, (uint32_t)n_arms, record_start, record_len,
                        (size_t)n_records, margin, min_depth);
    });
}

extern "C" void asgart_mask_counts(const asgart_mask *r, uint64_t *n_intervals, uint64_t *masked_bases, uint64_t *max_depth) {
    if (n_intervals) *n_intervals = r ? r->bounds.size() / 2 : 0;
    if (masked_bases) *masked_bases = r ? r->masked : 0;
    if (max_depth) *max_depth = r ? r->max_depth : 0;
}

extern "C" void asgart_mask_copy(const asgart_mask *r, uint64_t *intervals) {
    if (r) give(intervals, r->bounds);
}

extern "C" int32_t asgart_mask_timings(const asgart_mask *r, double *ms3) {
    return copy_ms3("asgart_mask_timings", r, ms3);
}

extern "C" void asgart_mask_free(asgart_mask *r) { delete r; }

extern "C" void asgart_mask_geometry(uint64_t *block_threads) {
    if (block_threads) *block_threads = kBlock;
}
