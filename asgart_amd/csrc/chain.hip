// chain.hip -- chaining: the collinear duplications of a result joined into the pairs they are pieces of:
// asgart_chain_duplications and its handle.  The rule is stated once, in include/asgart_hip.h; asgart_amd/chain.py:
// chain_host is the readable statement of it, and it does not cut.
//
// Nothing of the reference does this.  The work has a serial core, a dynamic programme over the anchors of a group in
// (pl, pr, q) order; what makes it device work is what the search does with its segments: the ranks are cut where no link
// can cross, and a wave walks each piece.
//
// Stages, all on one stream; two counts are read back at the very end:
//   order      three stable radix sorts of the ordinals: by pr, then by pl, then by the packed group (cl, cr, fl); the
//              anchors gathered into that order (the rank order), so that neighbouring lanes read neighbouring records
//   cut        the segmented inclusive max-scan of the left ends that groups.hip has (tool_base.hpp: KeyEnd, SegmentedMax,
//              sat_add): rank i opens a segment iff it is the first of its group or pl_i > sat(M + max_gap), M the largest
//              el of the earlier ranks of its group.  A link j -> i needs pl_i - el_j <= max_gap, so none crosses; starts
//              increase along the ranks, so none reaches an anchor further behind either.  The segments sorted by length,
//              the longest first
//   walk       chain_segments_kernel, one wave (one workgroup of 64) per segment, three sweeps with trip counts known
//              before they start, a fence between them:
//                forward    f and pred.  Anchor i's record is broadcast from the chunk of 64 the wave loaded together; lane d
//                           of a round evaluates the link from rank i - 1 - d, a 64-lane max-reduction finds the best
//                           score and a ballot of the lanes that hold it the NEAREST of them (the lowest lane; an earlier
//                           round wins a tie with a later one), so the tie-break is one scalar instruction
//                backward   g and succ, the mirror image: lane d looks at rank i + 1 + d, which is a child iff its pred
//                           is i; the lowest lane of the largest g is the child of the smallest rank
//                forward    link, the head of every anchor and its term: 64 anchors at a time, each lane one; heads within
//                           the chunk by six rounds of pointer doubling, heads of earlier chunks from the ring
//              The window (f, then g; the heads in the third sweep) lives in an LDS ring of 1024 entries, 8 KiB, for
//              H > 64, and for H <= 64 -- 64 included: one round is exactly the wave -- in registers, as a wave-wide shift
//              by one lane per anchor, with the starts and ends of the window's anchors beside it.
//              No spin-wait, no dependence between workgroups, no atomic retry loop
//   number     per anchor f, pred, link in ordinal order; the smallest ordinal of every chain by one atomicMin per anchor at
//              its head; the flags "q is the smallest of its chain", their exclusive scan numbers the chains
//   members    the ranks sorted stably by chain: order; chain_offsets by bisection in the sorted keys; chain_score from the
//              exclusive plus-scan of the terms in that order, one difference per chain (sums mod 2^64 of values whose true
//              sum is below 2^63)
#include "chain_dev.hpp"
#include "tool_base.hpp"

namespace asgart {
namespace {

constexpr uint32_t kBlock = 256;  // threads per workgroup of the elementwise kernels; a multiple of the wave size
constexpr uint32_t kRingMask = kChainMaxLookback - 1;

using GroupEnd = KeyEnd<uint64_t>;  // (packed group, el) of a rank

// ---- order ----------------------------------------------------------------------------------------------------------
// the keys of the first two passes: where the right (side 1), then the left (side 0) arm of duplication q starts
struct ChainStart {
    const uint64_t *__restrict__ chr_pos;
    uint32_t side;
    __device__ uint64_t operator()(uint32_t q) const { return chr_pos[2 * (size_t)q + side]; }
};

__global__ __launch_bounds__(kBlock) void chain_gather_kernel(const uint32_t *__restrict__ r_q,
                                                             const uint64_t *__restrict__ group_key,
                                                             const uint64_t *__restrict__ chr_pos,
                                                             const uint64_t *__restrict__ length, uint32_t n,
                                                             ChainAnchor *__restrict__ r_anchor, GroupEnd *__restrict__ pair) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t q = r_q[i];
    const ChainAnchor a{chr_pos[2 * q], chr_pos[2 * q + 1], length[2 * q], length[2 * q + 1]};
    r_anchor[i] = a;
    pair[i] = GroupEnd{a.pl + a.ll, group_key[i]};  // (the host has refused a sum that wraps)
}

// ---- cut ------------------------------------------------------------------------------------------------------------
// run[i - 1] is the largest el of all earlier ranks of rank i's group, where there is one; slot n closes the scan
__global__ __launch_bounds__(kBlock) void chain_heads_kernel(const GroupEnd *__restrict__ run,
                                                            const ChainAnchor *__restrict__ r_anchor, uint32_t n,
                                                            uint64_t max_gap, uint32_t *__restrict__ head) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    uint32_t h = i < n ? 1u : 0u;
    if (i > 0 && i < n) {
        const GroupEnd before = run[i - 1];
        h = (before.key != run[i].key || r_anchor[i].pl > sat_add(before.end, max_gap)) ? 1u : 0u;
    }
    head[i] = h;
}

// seg_start[k] of segment k, and the closing entry n behind the last
__global__ __launch_bounds__(kBlock) void chain_open_kernel(const uint32_t *__restrict__ head,
                                                           const uint32_t *__restrict__ rank, uint32_t n,
                                                           uint32_t *__restrict__ seg_start) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n || head[i]) seg_start[rank[i]] = i;
}

// the sort key of segment k: its length complemented, so that the longest come first; the slots behind the last segment
// sort behind every segment (a length is at least 1)
struct ChainLengthKey {
    const uint32_t *__restrict__ seg_start, *__restrict__ n_seg;
    __device__ uint32_t operator()(uint32_t k) const { return k < *n_seg ? ~(seg_start[k + 1] - seg_start[k]) : ~0u; }
};

// ---- walk -----------------------------------------------------------------------------------------------------------
struct ChainWalk {
    const ChainAnchor *r_anchor;  // the anchors in rank order
    const uint8_t *flags;
    const uint32_t *r_q;
    const uint32_t *seg_start, *seg_order, *n_seg;
    int64_t *r_f, *r_term;
    int32_t *r_pred, *r_succ, *r_link;
    uint32_t *r_head;
    uint64_t max_gap;
    uint32_t lookback;
};

__device__ inline ChainAnchor anchor_of_lane(const ChainAnchor &mine, uint32_t k) {
    return ChainAnchor{lane_value(mine.pl, k), lane_value(mine.pr, k), lane_value(mine.ll, k), lane_value(mine.rl, k)};
}

// One workgroup of one wave per segment, the longest segments in the first workgroups.  kRing: the window lives in the LDS
// ring (any lookback); otherwise in registers (lookback <= 64).  Every rank the kernel touches lies in [s, e), e <= n.
template <bool kRing>
__global__ __launch_bounds__(kChainLanes) void chain_segments_kernel(ChainWalk w) {
    __shared__ int64_t ring[kChainMaxLookback];
    if (blockIdx.x >= *w.n_seg) return;  // (the whole workgroup)
    const uint32_t seg = w.seg_order[blockIdx.x];
    const uint32_t s = w.seg_start[seg], e = w.seg_start[seg + 1], lane = threadIdx.x, H = w.lookback;
    const bool reversed = (w.flags[w.r_q[s]] & 1) != 0;  // one group, one geometry
    const ChainAnchor none{0, 0, 1, 1};

    // forward: f and pred.  Lane d of the register window holds rank i - 1 - d
    {
        uint64_t w_pl = 0, w_el = 0, w_pr = 0, w_er = 0;
        int64_t w_f = 0;
        for (uint32_t b = s; b < e; b += kChainLanes) {
            const uint32_t cnt = e - b < kChainLanes ? e - b : kChainLanes, idx = b + lane;
            const ChainAnchor mine = idx < e ? w.r_anchor[idx] : none;
            int64_t my_f = 0;
            int32_t my_pred = -1;
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t i = b + k, n_win = i - s < H ? i - s : H;
                const ChainAnchor cur = anchor_of_lane(mine, k);
                int64_t best = kNoScore;
                uint32_t best_d = 0;
                if (!kRing) {
                    int64_t cand = kNoScore, t;
                    if (lane < n_win && chain_link(w_pl, w_el, w_pr, w_er, cur, reversed, w.max_gap, &t)) cand = w_f + t;
                    best = wave_max(cand);
                    if (best != kNoScore) best_d = first_lane(cand == best);
                } else {
                    for (uint32_t r0 = 0; r0 < n_win; r0 += kChainLanes) {
                        const uint32_t d = r0 + lane;
                        int64_t cand = kNoScore, t;
                        if (d < n_win) {
                            const uint32_t j = i - 1 - d;
                            const ChainAnchor a = w.r_anchor[j];
                            if (chain_link(a.pl, a.pl + a.ll, a.pr, a.pr + a.rl, cur, reversed, w.max_gap, &t))
                                cand = ring[j & kRingMask] + t;
                        }
                        const int64_t m = wave_max(cand);
                        if (m > best) {  // (strictly: a nearer round keeps a tie)
                            best = m;
                            best_d = r0 + first_lane(cand == m);
                        }
                    }
                }
                const int64_t base = (int64_t)(cur.ll < cur.rl ? cur.ll : cur.rl);
                const bool linked = best > base;
                const int64_t f_i = linked ? best : base;
                if (lane == k) {
                    my_f = f_i;
                    my_pred = linked ? (int32_t)(i - 1 - best_d) : -1;
                }
                if (kRing) {
                    if (lane == 0) ring[i & kRingMask] = f_i;
                    __syncthreads();
                } else {
                    w_pl = shift_in(w_pl, cur.pl);
                    w_el = shift_in(w_el, cur.pl + cur.ll);
                    w_pr = shift_in(w_pr, cur.pr);
                    w_er = shift_in(w_er, cur.pr + cur.rl);
                    w_f = shift_in(w_f, f_i);
                }
            }
            if (idx < e) {
                w.r_f[idx] = my_f;
                w.r_pred[idx] = my_pred;
            }
        }
    }
    __threadfence();  // the lanes read each other's f and pred from here on
    __syncthreads();

    // backward: g and succ.  Lane d of the register window holds rank i + 1 + d
    {
        int32_t w_pred = -1;
        int64_t w_g = 0;
        for (uint32_t c = (e - s + kChainLanes - 1) / kChainLanes; c-- > 0;) {
            const uint32_t b = s + c * kChainLanes, cnt = e - b < kChainLanes ? e - b : kChainLanes, idx = b + lane;
            const int64_t my_f = idx < e ? w.r_f[idx] : 0;
            const int32_t my_pred = idx < e ? w.r_pred[idx] : -1;
            int32_t my_succ = -1;
            for (uint32_t k = cnt; k-- > 0;) {
                const uint32_t i = b + k, n_win = e - 1 - i < H ? e - 1 - i : H;
                const int64_t f_i = lane_value(my_f, k);
                const int32_t pred_i = lane_value(my_pred, k);
                int64_t best = kNoScore;
                uint32_t best_d = 0;
                if (!kRing) {
                    const int64_t cand = (lane < n_win && w_pred == (int32_t)i) ? w_g : kNoScore;
                    best = wave_max(cand);
                    if (best != kNoScore) best_d = first_lane(cand == best);
                } else {
                    for (uint32_t r0 = 0; r0 < n_win; r0 += kChainLanes) {
                        const uint32_t d = r0 + lane;
                        int64_t cand = kNoScore;
                        if (d < n_win) {
                            const uint32_t child = i + 1 + d;
                            if (w.r_pred[child] == (int32_t)i) cand = ring[child & kRingMask];
                        }
                        const int64_t m = wave_max(cand);
                        if (m > best) {  // (strictly: a round of smaller ranks keeps a tie)
                            best = m;
                            best_d = r0 + first_lane(cand == m);
                        }
                    }
                }
                const bool parent = best != kNoScore;
                const int64_t g_i = parent && best > f_i ? best : f_i;
                if (lane == k) my_succ = parent ? (int32_t)(i + 1 + best_d) : -1;
                if (kRing) {
                    if (lane == 0) ring[i & kRingMask] = g_i;
                    __syncthreads();
                } else {
                    w_pred = shift_in(w_pred, pred_i);
                    w_g = shift_in(w_g, g_i);
                }
            }
            if (idx < e) w.r_succ[idx] = my_succ;
        }
    }
    __threadfence();  // the lanes read each other's succ
    __syncthreads();

    // forward: link, head and term, a lane per anchor.  The heads of the last 1024 ranks live in the ring
    uint32_t *const head_ring = reinterpret_cast<uint32_t *>(ring);
    for (uint32_t b = s; b < e; b += kChainLanes) {
        const uint32_t idx = b + lane;
        const bool in = idx < e;
        int32_t link = -1;
        int64_t term = 0;
        if (in) {
            const int32_t p = w.r_pred[idx];
            if (p >= 0 && w.r_succ[p] == (int32_t)idx) link = p;
            const ChainAnchor me = w.r_anchor[idx];
            term = (int64_t)(me.ll < me.rl ? me.ll : me.rl);
            if (link >= 0) {
                const ChainAnchor a = w.r_anchor[link];
                (void)chain_link(a.pl, a.pl + a.ll, a.pr, a.pr + a.rl, me, reversed, w.max_gap, &term);
            }
        }
        bool done = link < 0 || (uint32_t)link < b;
        uint32_t head = link < 0 ? idx : ((uint32_t)link < b ? head_ring[(uint32_t)link & kRingMask] : 0u);
        int32_t at = done ? (int32_t)lane : (int32_t)((uint32_t)link - b);  // the lane that knows more
        // after round r every lane at most 2^r - 1 kept links behind a known head knows its own; a chunk has 64 lanes
        for (int r = 0; r < 6; ++r) {
            const int src = done ? (int)lane : at;
            const int src_done = __shfl((int)done, src);
            const uint32_t src_head = __shfl(head, src);
            const int32_t src_at = __shfl(at, src);
            if (!done) {
                if (src_done) {
                    head = src_head;
                    done = true;
                } else {
                    at = src_at;
                }
            }
        }
        __syncthreads();  // the ring is read before it is written
        if (in) {
            head_ring[idx & kRingMask] = head;
            w.r_link[idx] = link;
            w.r_head[idx] = head;
            w.r_term[idx] = term;
        }
        __syncthreads();
    }
}

// ---- number, members ------------------------------------------------------------------------------------------------
__device__ inline int32_t ordinal_of(const uint32_t *__restrict__ r_q, int32_t rank) {
    return rank < 0 ? -1 : (int32_t)r_q[rank];
}

__global__ __launch_bounds__(kBlock) void chain_scatter_kernel(const uint32_t *__restrict__ r_q,
                                                              const int64_t *__restrict__ r_f,
                                                              const int32_t *__restrict__ r_pred,
                                                              const int32_t *__restrict__ r_link,
                                                              const uint32_t *__restrict__ r_head, uint32_t n,
                                                              int64_t *__restrict__ f, int32_t *__restrict__ pred,
                                                              int32_t *__restrict__ link, uint32_t *smallest) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t q = r_q[i];
    f[q] = r_f[i];
    pred[q] = ordinal_of(r_q, r_pred[i]);
    link[q] = ordinal_of(r_q, r_link[i]);
    atomicMin(smallest + r_head[i], q);  // (indexed by the head's rank)
}

// first[q] = q is the smallest member of its chain; slot n closes the scan
__global__ __launch_bounds__(kBlock) void chain_first_kernel(const uint32_t *__restrict__ r_q,
                                                            const uint32_t *__restrict__ r_head,
                                                            const uint32_t *__restrict__ smallest, uint32_t n,
                                                            uint32_t *__restrict__ first) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        first[n] = 0u;
        return;
    }
    const uint32_t q = r_q[i];
    first[q] = smallest[r_head[i]] == q ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void chain_number_kernel(const uint32_t *__restrict__ r_q,
                                                             const uint32_t *__restrict__ r_head,
                                                             const uint32_t *__restrict__ smallest,
                                                             const uint32_t *__restrict__ number, uint32_t n,
                                                             uint32_t *__restrict__ chain, uint32_t *__restrict__ r_chain,
                                                             uint32_t *__restrict__ r_self) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = number[smallest[r_head[i]]];
    chain[r_q[i]] = c;
    r_chain[i] = c;
    r_self[i] = i;
}

// the members chain by chain: the ordinal and the term of every sorted rank; slot n closes the scan of the terms
__global__ __launch_bounds__(kBlock) void chain_members_kernel(const uint32_t *__restrict__ sorted_rank,
                                                              const uint32_t *__restrict__ r_q,
                                                              const int64_t *__restrict__ r_term, uint32_t n,
                                                              uint32_t *__restrict__ order, uint64_t *__restrict__ term) {
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
    if (x > n) return;
    if (x == n) {
        term[n] = 0;
        return;
    }
    const uint32_t i = sorted_rank[x];
    order[x] = r_q[i];
    term[x] = (uint64_t)r_term[i];
}

// chain_offsets[c], c in [0, n_chains]: the first sorted rank whose chain is >= c; the score is a difference of the scan
__global__ __launch_bounds__(kBlock) void chain_offsets_kernel(const uint32_t *__restrict__ sorted_chain, uint32_t n,
                                                              const uint32_t *__restrict__ total,
                                                              const uint64_t *__restrict__ term_before,
                                                              uint64_t *__restrict__ offsets, int64_t *__restrict__ score) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_chains = *total;
    if (c > n_chains) return;
    const uint32_t at = first_at_least(sorted_chain, n, c);
    offsets[c] = at;
    if (c < n_chains) score[c] = (int64_t)(term_before[first_at_least(sorted_chain, n, c + 1u)] - term_before[at]);
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_chains {
    std::vector<int64_t> f, chain_score;
    std::vector<int32_t> pred, link;
    std::vector<uint32_t> chain, order;
    std::vector<uint64_t> chain_offsets;
    uint64_t n_sds = 0, n_segments = 0;
    double ms[3] = {0, 0, 0};
};

namespace {

const char *const kWho = "asgart_chain_duplications";

struct ChainWork : ToolWork {
    DevBuf &chr = buf(), &chr_pos = buf(), &length = buf(), &flags = buf();
    DevBuf &ord0 = buf(), &ord1 = buf(), &ord2 = buf(), &r_q = buf(), &key_a = buf(), &key_b = buf(), &group_key = buf();
    DevBuf &r_anchor = buf(), &pair = buf(), &run = buf(), &head = buf(), &rank = buf(), &seg_start = buf();
    DevBuf &len_key = buf(), &len_sorted = buf(), &seg0 = buf(), &seg_order = buf();
    DevBuf &r_f = buf(), &r_term = buf(), &r_pred = buf(), &r_succ = buf(), &r_link = buf(), &r_head = buf();
    DevBuf &f = buf(), &pred = buf(), &link = buf(), &smallest = buf(), &first = buf(), &number = buf(), &chain = buf();
    DevBuf &r_chain = buf(), &r_self = buf(), &sorted_chain = buf(), &sorted_rank = buf(), &order = buf(), &term = buf();
    DevBuf &term_before = buf(), &offsets = buf(), &score = buf();
};

const char *side_of(int arm) { return arm ? "right" : "left"; }

int32_t check_arguments(const int32_t *chr, const uint64_t *chr_pos, const uint64_t *length, const uint8_t *flags,
                        int64_t n_sds, int64_t n_names, uint64_t max_gap, int32_t lookback, asgart_chains **out) {
    if (!out) {
        set_error("%s: bad argument (out is NULL)", kWho);
        return ASGART_E_ARG;
    }
    if (n_sds < 0 || n_names < 0) {
        set_error("%s: a negative count (n_sds = %lld, n_names = %lld)", kWho, (long long)n_sds, (long long)n_names);
        return ASGART_E_ARG;
    }
    if (n_sds > 0 && (!chr || !chr_pos || !length || !flags)) {
        set_error("%s: a NULL anchor array with n_sds = %lld", kWho, (long long)n_sds);
        return ASGART_E_ARG;
    }
    if (lookback < 1 || lookback > (int32_t)kChainMaxLookback) {
        set_error("%s: lookback %d is outside 1 .. %u", kWho, (int)lookback, kChainMaxLookback);
        return ASGART_E_ARG;
    }
    if (max_gap >= ((uint64_t)1 << 62)) {
        set_error("%s: max_gap %llu is 2^62 or more", kWho, (unsigned long long)max_gap);
        return ASGART_E_ARG;
    }
    if (n_sds >= ((int64_t)1 << 31)) {
        set_error("%s: 2^31 duplications and more are not supported", kWho);
        return ASGART_E_CAP;
    }
    for (int64_t q = 0; q < n_sds; ++q) {
        for (int arm = 0; arm < 2; ++arm) {
            const int64_t j = 2 * q + arm;
            if (chr[j] < 0 || (int64_t)chr[j] >= n_names) {
                set_error("%s: duplication %lld (%s) has the name id %d, outside [0, %lld)", kWho, (long long)q, side_of(arm),
                          (int)chr[j], (long long)n_names);
                return ASGART_E_ARG;
            }
            if (length[j] == 0) {
                set_error("%s: duplication %lld (%s) has length 0: an empty arm makes no progress", kWho, (long long)q,
                          side_of(arm));
                return ASGART_E_ARG;
            }
            if (chr_pos[j] + length[j] < chr_pos[j]) {
                set_error("%s: duplication %lld (%s): position %llu + length %llu wraps past 2^64", kWho, (long long)q,
                          side_of(arm), (unsigned long long)chr_pos[j], (unsigned long long)length[j]);
                return ASGART_E_ARG;
            }
            if (length[j] >= ((uint64_t)1 << 32)) {
                set_error("%s: duplication %lld (%s) has %llu bases: arms of 2^32 bases and more are not supported", kWho,
                          (long long)q, side_of(arm), (unsigned long long)length[j]);
                return ASGART_E_CAP;
            }
        }
        if (flags[q] > 3) {
            set_error("%s: duplication %lld has the flag byte %u, above 3", kWho, (long long)q, (unsigned)flags[q]);
            return ASGART_E_ARG;
        }
    }
    return 0;
}

int32_t run_chain(ChainWork &w, asgart_chains *res, const int32_t *chr, const uint64_t *chr_pos, const uint64_t *length,
                  const uint8_t *flags, uint32_t n, uint64_t n_names, uint64_t max_gap, uint32_t lookback) {
    RC_TRY(w.open(3));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.chr, chr, (size_t)n * 8));
    RC_TRY(w.upload(w.chr_pos, chr_pos, (size_t)n * 16));
    RC_TRY(w.upload(w.length, length, (size_t)n * 16));
    RC_TRY(w.upload(w.flags, flags, n));
    for (DevBuf *b : {&w.ord0, &w.ord1, &w.ord2, &w.r_q, &w.len_key, &w.len_sorted, &w.seg0, &w.seg_order, &w.r_pred, &w.r_succ,
                      &w.r_link, &w.r_head, &w.pred, &w.link, &w.smallest, &w.chain, &w.r_chain, &w.r_self, &w.sorted_chain,
                      &w.sorted_rank, &w.order})
        RC_TRY(b->reserve((size_t)n * 4));
    for (DevBuf *b : {&w.key_a, &w.key_b, &w.group_key, &w.r_f, &w.r_term, &w.f, &w.score}) RC_TRY(b->reserve((size_t)n * 8));
    RC_TRY(w.r_anchor.reserve((size_t)n * sizeof(ChainAnchor)));
    for (DevBuf *b : {&w.pair, &w.run}) RC_TRY(b->reserve((size_t)n * sizeof(GroupEnd)));
    // one closing entry each: the exclusive scans over n + 1 end in the totals, seg_start and offsets in n
    for (DevBuf *b : {&w.head, &w.rank, &w.seg_start, &w.first, &w.number}) RC_TRY(b->reserve(((size_t)n + 1) * 4));
    for (DevBuf *b : {&w.term, &w.term_before, &w.offsets}) RC_TRY(b->reserve(((size_t)n + 1) * 8));
    HIP_TRY(hipMemsetAsync(w.smallest.p, 0xff, (size_t)n * 4, s));
    HIP_TRY(hipEventRecord(w.ev[1], s));

    const unsigned grid = blocks_for(n, kBlock), grid1 = blocks_for((uint64_t)n + 1, kBlock);
    uint32_t *head = w.head.as<uint32_t>(), *rank = w.rank.as<uint32_t>(), *number = w.number.as<uint32_t>();
    uint32_t *r_q = w.r_q.as<uint32_t>();
    const unsigned name_bits = bits_for(std::min<uint64_t>(n_names, (uint64_t)1 << 31));  // (ids are below 2^31)
    // by pr, then by pl, then by the packed group (cl, cr, fl)
    RC_TRY(w.order_pass<uint64_t>(ChainStart{w.chr_pos.as<uint64_t>(), 1}, w.key_a, w.key_b, w.ord0, kNoOrder, w.ord1, n, 64));
    RC_TRY(w.order_pass<uint64_t>(ChainStart{w.chr_pos.as<uint64_t>(), 0}, w.key_a, w.key_b, w.ord1, kOrdered, w.ord2, n, 64));
    RC_TRY(w.order_pass<uint64_t>(ChainGroupKey{w.chr.as<int32_t>(), w.flags.as<uint8_t>(), name_bits}, w.key_a, w.group_key,
                                  w.ord2, kOrdered, w.r_q, n, 2 * name_bits + 2));
    chain_gather_kernel<<<grid, kBlock, 0, s>>>(r_q, w.group_key.as<uint64_t>(), w.chr_pos.as<uint64_t>(),
                                                w.length.as<uint64_t>(), n, w.r_anchor.as<ChainAnchor>(),
                                                w.pair.as<GroupEnd>());
    HIP_TRY(hipGetLastError());

    RC_TRY(w.segmented_max_scan(w.pair.as<GroupEnd>(), w.run.as<GroupEnd>(), n));
    chain_heads_kernel<<<grid1, kBlock, 0, s>>>(w.run.as<GroupEnd>(), w.r_anchor.as<ChainAnchor>(), n, max_gap, head);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(head, rank, (size_t)n + 1));
    chain_open_kernel<<<grid1, kBlock, 0, s>>>(head, rank, n, w.seg_start.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    // the segments by length, the longest first: an ordering of its own, one pass
    RC_TRY(w.order_pass<uint32_t>(ChainLengthKey{w.seg_start.as<uint32_t>(), rank + n}, w.len_key, w.len_sorted, w.seg0, kNoOrder,
                                  w.seg_order, n, 32));

    const ChainWalk walk{w.r_anchor.as<ChainAnchor>(), w.flags.as<uint8_t>(), r_q, w.seg_start.as<uint32_t>(),
                         w.seg_order.as<uint32_t>(), rank + n, w.r_f.as<int64_t>(), w.r_term.as<int64_t>(),
                         w.r_pred.as<int32_t>(), w.r_succ.as<int32_t>(), w.r_link.as<int32_t>(), w.r_head.as<uint32_t>(),
                         max_gap, lookback};
    // a workgroup per possible segment: those behind the last leave at once (the count stays on the device)
    if (lookback <= kChainLanes)
        chain_segments_kernel<false><<<n, kChainLanes, 0, s>>>(walk);
    else
        chain_segments_kernel<true><<<n, kChainLanes, 0, s>>>(walk);
    HIP_TRY(hipGetLastError());

    chain_scatter_kernel<<<grid, kBlock, 0, s>>>(r_q, w.r_f.as<int64_t>(), w.r_pred.as<int32_t>(), w.r_link.as<int32_t>(),
                                                 w.r_head.as<uint32_t>(), n, w.f.as<int64_t>(), w.pred.as<int32_t>(),
                                                 w.link.as<int32_t>(), w.smallest.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    chain_first_kernel<<<grid1, kBlock, 0, s>>>(r_q, w.r_head.as<uint32_t>(), w.smallest.as<uint32_t>(), n,
                                                w.first.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.first.as<uint32_t>(), number, (size_t)n + 1));
    chain_number_kernel<<<grid, kBlock, 0, s>>>(r_q, w.r_head.as<uint32_t>(), w.smallest.as<uint32_t>(), number, n,
                                                w.chain.as<uint32_t>(), w.r_chain.as<uint32_t>(), w.r_self.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.sort_pairs(w.r_chain.as<uint32_t>(), w.sorted_chain.as<uint32_t>(), w.r_self.as<uint32_t>(),
                        w.sorted_rank.as<uint32_t>(), n, bits_for(n)));
    chain_members_kernel<<<grid1, kBlock, 0, s>>>(w.sorted_rank.as<uint32_t>(), r_q, w.r_term.as<int64_t>(), n,
                                                  w.order.as<uint32_t>(), w.term.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.term.as<uint64_t>(), w.term_before.as<uint64_t>(), (size_t)n + 1));
    chain_offsets_kernel<<<grid1, kBlock, 0, s>>>(w.sorted_chain.as<uint32_t>(), n, number + n, w.term_before.as<uint64_t>(),
                                                  w.offsets.as<uint64_t>(), w.score.as<int64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[2], s));

    uint32_t n_seg = 0, n_chains = 0;  // the count that sizes the output, and the one no array shows
    HIP_TRY(read_back(&n_seg, rank + n, 4, s));
    HIP_TRY(read_back(&n_chains, number + n, 4, s));
    if (n_seg == 0 || n_seg > n || n_chains == 0 || n_chains > n) {
        set_error("%s: %u segments and %u chains of %u duplications", kWho, n_seg, n_chains, n);
        return ASGART_E_HIP;
    }
    res->n_sds = n;
    res->n_segments = n_seg;
    w.start_copy_back();
    RC_TRY(w.fetch(res->f, w.f, n));
    RC_TRY(w.fetch(res->pred, w.pred, n));
    RC_TRY(w.fetch(res->link, w.link, n));
    RC_TRY(w.fetch(res->chain, w.chain, n));
    RC_TRY(w.fetch(res->order, w.order, n));
    RC_TRY(w.fetch(res->chain_offsets, w.offsets, (size_t)n_chains + 1));
    RC_TRY(w.fetch(res->chain_score, w.score, n_chains));
    HIP_TRY(stream_sync(s));
    return w.figures(res->ms);
}

}  // namespace

extern "C" int32_t asgart_chain_duplications(int32_t device, const int32_t *chr, const uint64_t *chr_pos,
                                             const uint64_t *length, const uint8_t *flags, int64_t n_sds, int64_t n_names,
                                             uint64_t max_gap, int32_t lookback, asgart_chains **out) {
    if (out) *out = nullptr;
    RC_TRY(check_arguments(chr, chr_pos, length, flags, n_sds, n_names, max_gap, lookback, out));
    RC_TRY(use_device(kWho, device));
    if (n_sds == 0) {  // no anchors, no chains; nothing is launched
        *out = new asgart_chains;
        (*out)->chain_offsets.assign(1, 0);
        return 0;
    }
    return run_tool<ChainWork>(out, [&](ChainWork &w, asgart_chains *res) {
        return run_chain(w, res, chr, chr_pos, length, flags, (uint32_t)n_sds, (uint64_t)n_names, max_gap, (uint32_t)lookback);
    });
}

extern "C" void asgart_chains_counts(const asgart_chains *r, uint64_t *n_sds, uint64_t *n_chains, uint64_t *n_links,
                                     uint64_t *n_segments) {
    if (n_sds) *n_sds = r ? r->n_sds : 0;
    if (n_chains) *n_chains = r ? r->chain_score.size() : 0;
    if (n_links) *n_links = r ? r->n_sds - r->chain_score.size() : 0;  // every member but the head has one kept link
    if (n_segments) *n_segments = r ? r->n_segments : 0;
}

extern "C" void asgart_chains_copy(const asgart_chains *r, int64_t *f, int32_t *pred, int32_t *link, uint32_t *chain,
                                   uint32_t *order, uint64_t *chain_offsets, int64_t *chain_score) {
    if (!r) return;
    give(f, r->f);
    give(pred, r->pred);
    give(link, r->link);
    give(chain, r->chain);
    give(order, r->order);
    give(chain_offsets, r->chain_offsets);
    give(chain_score, r->chain_score);
}

extern "C" int32_t asgart_chains_timings(const asgart_chains *r, double *ms3) {
    return copy_ms3("asgart_chains_timings", r, ms3);
}

extern "C" void asgart_chains_free(asgart_chains *r) { delete r; }

extern "C" void asgart_chain_geometry(uint64_t *block_threads, uint64_t *window_lanes, uint64_t *max_lookback) {
    if (block_threads) *block_threads = kBlock;
    if (window_lanes) *window_lanes = kChainLanes;
    if (max_lookback) *max_lookback = kChainMaxLookback;
}
