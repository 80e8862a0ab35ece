// plot.hip -- the filters of asgart-plot on family arrays and flattened feature tracks: asgart_plot_filter and its handle.
//
// Replaces, for a result held as arrays, the per-duplication part of reference src/bin/asgart-plot.rs:463-481: the retains
// of --min-length (:463-465, the LONGER arm decides) and of --min-identity / --max-identity (:467-469, f32 compares), and
// the three feature filters filter_families_in_features (:20-70), filter_duplicons_in_features (:72-119) and
// filter_features_in_sds (:121-163).  The reference answers those three by testing every duplication against every
// position of every feature of every track with `_overlap` (:25-30), in one thread.  They are interval joins:
//
//   A window (start - threshold, length + 2 * threshold) or an arm (position, length) is PROPER when nothing in it wraps
//   mod 2^64: first <= last as numbers.  For two proper intervals `_overlap` is `xs <= ye && ys <= xe`, and since
//   ye < xs implies ys <= xe, "some target overlaps x" is  #{ys <= xe} - #{ye < xs} > 0:  two radix sorts of the proper
//   targets' firsts and lasts, two bisections per query.  The improper ones (a feature closer to 0 than the threshold, an
//   arm that ends past 2^64) keep the reference's behaviour bit for bit through a second kernel that evaluates the LITERAL
//   predicate on wrapped values: every query against the improper targets, the improper queries against the proper
//   targets.  options.force_literal marks every target improper, so that tests run both paths on one input.
//
// For filter_families / filter_duplicons the queries are the arms of the duplications still alive and the targets the
// windows of the positions in front of the first unresolved one, U (the reference walks the positions in flat order,
// returns at the first match and panics when it gets to U).  For filter_features the roles swap: the targets are the
// surviving arms, the queries the windows of all resolved positions.
//
// Family sizes are differences of a scan over duplications at the family's two offsets, as in slice.hip: an empty family,
// one larger than a workgroup and one larger than 65 535 are the same case.  "First stop of a feature" is the same trick on
// the scan of the stop flags.  Survivors keep the input order.  Lists are appended to with one atomic per wave; their order
// differs from call to call and no result depends on it.  The error ordinals are minima (atomicMin), as slice.hip's err.
#include "tool_base.hpp"

namespace asgart {
namespace {

constexpr uint32_t kBlock = 256;  // threads per workgroup, every kernel
constexpr uint32_t kTile = 512;   // targets staged in LDS per round of the literal kernel (8 KiB)
constexpr uint32_t kNone = 0xFFFFFFFFu;

// An interval list: first, last (both as computed, wrapping), proper byte, owner (the duplication or the position).
struct Intervals {
    uint64_t *s, *e;
    uint8_t *proper;
    uint32_t *owner;
};

// the literal `_overlap` (asgart-plot.rs:25-30) on the values the reference computes
__device__ inline bool overlap_literal(uint64_t xs, uint64_t xe, uint64_t ys, uint64_t ye) {
    return (xs >= ys && xs <= ye) || (ys >= xs && ys <= xe);
}

// One slot of a list per lane that wants one, one atomic per wave.  Every lane of the wave must call it.
__device__ inline uint32_t wave_append(bool want, uint32_t *counter) {
    const unsigned long long mask = __ballot(want);
    if (mask == 0) return 0;
    const uint32_t lane = __lane_id();
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// --min-length (the longer arm) and the identity range in f32: a NaN fails both compares
__global__ __launch_bounds__(kBlock) void plot_flags_kernel(const asgart_proto_sd *__restrict__ sds,
                                                           const float *__restrict__ identity, uint32_t n,
                                                           asgart_plot_options opt, uint32_t *__restrict__ alive) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    if (opt.has_min_length) {
        const uint64_t ll = sds[i].left_length, rl = sds[i].right_length;
        ok = (ll > rl ? ll : rl) >= opt.min_length;
    }
    if (opt.has_identity) {
        const float v = identity[i];
        ok = ok && opt.min_identity <= v && v <= opt.max_identity;
    }
    alive[i] = ok ? 1u : 0u;
}

// both arms of every duplication alive, at slots 2 * rank and 2 * rank + 1
__global__ __launch_bounds__(kBlock) void plot_emit_arms_kernel(const asgart_proto_sd *__restrict__ sds, uint32_t n,
                                                               const uint32_t *__restrict__ alive,
                                                               const uint32_t *__restrict__ rank, Intervals out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !alive[i]) return;
    const asgart_proto_sd d = sds[i];
    const uint32_t j = 2 * rank[i];
    const uint64_t le = d.left + d.left_length, re = d.right + d.right_length;
    out.s[j] = d.left;
    out.e[j] = le;
    out.proper[j] = le >= d.left;
    out.owner[j] = i;
    out.s[j + 1] = d.right;
    out.e[j + 1] = re;
    out.proper[j + 1] = re >= d.right;
    out.owner[j + 1] = i;
}

// the window of every resolved position in [0, limit), appended
__global__ __launch_bounds__(kBlock) void plot_emit_windows_kernel(const uint64_t *__restrict__ start,
                                                                  const uint64_t *__restrict__ length,
                                                                  const uint8_t *__restrict__ resolved, uint32_t limit,
                                                                  uint64_t t, Intervals out, uint32_t *__restrict__ count) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const bool want = p < limit && resolved[p] != 0;
    uint64_t st = 0, ln = 0;
    if (want) {
        st = start[p];
        ln = length[p];
    }
    const uint64_t ws = st - t, wl = ln + 2 * t, we = ws + wl;
    const uint32_t j = wave_append(want, count);
    if (!want) return;
    out.s[j] = ws;
    out.e[j] = we;
    out.proper[j] = st >= t && t <= 0x7FFFFFFFFFFFFFFFull && wl >= ln && we >= ws;
    out.owner[j] = p;
}

// targets -> the proper ones (firsts and lasts, for the sorts and as pairs) and the improper ones
__global__ __launch_bounds__(kBlock) void plot_split_kernel(Intervals in, uint32_t n, uint32_t force_literal,
                                                           uint64_t *__restrict__ ps, uint64_t *__restrict__ pe,
                                                           uint64_t *__restrict__ is, uint64_t *__restrict__ ie,
                                                           uint32_t *__restrict__ counts) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < n;
    const bool proper = in_range && in.proper[i] && !force_literal;
    const uint32_t jp = wave_append(proper, counts);
    const uint32_t ji = wave_append(in_range && !proper, counts + 1);
    if (!in_range) return;
    if (proper) {
        ps[jp] = in.s[i];
        pe[jp] = in.e[i];
    } else {
        is[ji] = in.s[i];
        ie[ji] = in.e[i];
    }
}

// proper queries: two bisections in the sorted firsts and lasts of the proper targets; improper ones are appended
__global__ __launch_bounds__(kBlock) void plot_bisect_kernel(Intervals q, uint32_t nq,
                                                            const uint64_t *__restrict__ sorted_s,
                                                            const uint64_t *__restrict__ sorted_e, uint32_t nt,
                                                            uint32_t *__restrict__ hit, Intervals improper,
                                                            uint32_t *__restrict__ n_improper) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < nq;
    const bool proper = in_range && q.proper[i];
    const uint32_t j = wave_append(in_range && !proper, n_improper);
    if (!in_range) return;
    const uint64_t xs = q.s[i], xe = q.e[i];
    if (!proper) {
        improper.s[j] = xs;
        improper.e[j] = xe;
        improper.owner[j] = q.owner[i];
        return;
    }
    uint32_t lo = 0, hi = nt;  // #{ys <= xe}: the first sorted first above xe
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sorted_s[mid] <= xe) lo = mid + 1; else hi = mid;
    }
    const uint32_t starts = lo;
    lo = 0, hi = nt;           // #{ye < xs}: the first sorted last that is not below xs
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sorted_e[mid] < xs) lo = mid + 1; else hi = mid;
    }
    if (starts > lo) hit[q.owner[i]] = 1u;
}

// The literal predicate, one query per lane against every target: a tile of targets in LDS per round; a wave leaves a
// tile once all its lanes have matched (ballot), the workgroup leaves the loop once all its waves have.
__global__ __launch_bounds__(kBlock) void plot_literal_kernel(const uint64_t *__restrict__ qs,
                                                             const uint64_t *__restrict__ qe,
                                                             const uint32_t *__restrict__ qo, uint32_t nq,
                                                             const uint64_t *__restrict__ ts,
                                                             const uint64_t *__restrict__ te, uint32_t nt,
                                                             uint32_t *__restrict__ hit) {
    __shared__ uint64_t l_s[kTile], l_e[kTile];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < nq;
    const uint64_t xs = in_range ? qs[i] : 0, xe = in_range ? qe[i] : 0;
    bool done = !in_range, found = false;
    for (uint32_t base = 0; base < nt; base += kTile) {
        if (__syncthreads_and(done)) break;  // (also: the tile of the round before has been read by everyone)
        const uint32_t m = nt - base < kTile ? nt - base : kTile;
        for (uint32_t k = threadIdx.x; k < m; k += kBlock) {
            l_s[k] = ts[base + k];
            l_e[k] = te[base + k];
        }
        __syncthreads();
        for (uint32_t k = 0; k < m; ++k) {
            if (!done && overlap_literal(xs, xe, l_s[k], l_e[k])) found = done = true;
            if ((k & 15u) == 15u && __ballot(!done) == 0) break;
        }
    }
    if (found) hit[qo[i]] = 1u;
}

// after the join of filter_families: matched[i] = alive and hit; with an unresolved position U, the first duplication alive
// of a family that did not match is where the reference reaches U and panics
__global__ __launch_bounds__(kBlock) void plot_family_first_kernel(const uint64_t *__restrict__ offs, uint32_t n_fam,
                                                                  uint32_t n, const uint32_t *__restrict__ alive,
                                                                  const uint32_t *__restrict__ rank,
                                                                  const uint32_t *__restrict__ hit, uint32_t u,
                                                                  uint32_t *__restrict__ matched, uint32_t *__restrict__ err) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const bool a = alive[i] != 0, h = hit[i] != 0;
    matched[i] = (a && h) ? 1u : 0u;
    if (u != kNone && a && !h && rank[i] == rank[offs[segment_of(offs, n_fam, i)]]) atomicMin(err, u);
}

// family f stays iff one of its duplications matched; with a U (and no panic) iff it is not empty
__global__ __launch_bounds__(kBlock) void plot_family_keep_kernel(const uint64_t *__restrict__ offs, uint32_t n_fam,
                                                                 const uint32_t *__restrict__ rank,
                                                                 const uint32_t *__restrict__ rank_matched, uint32_t u,
                                                                 uint32_t *__restrict__ fam_keep) {
    const uint32_t f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_fam) return;
    const uint64_t a = offs[f], b = offs[f + 1];
    fam_keep[f] = (u != kNone ? rank[b] - rank[a] : rank_matched[b] - rank_matched[a]) > 0 ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void plot_family_apply_kernel(const uint64_t *__restrict__ offs, uint32_t n_fam,
                                                                  uint32_t n, const uint32_t *__restrict__ fam_keep,
                                                                  uint32_t *__restrict__ alive) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !alive[i]) return;
    if (!fam_keep[segment_of(offs, n_fam, i)]) alive[i] = 0u;
}

// after the join of filter_duplicons: a duplication that matched nothing goes; with a U it is where the reference panics
__global__ __launch_bounds__(kBlock) void plot_duplicons_kernel(uint32_t n, const uint32_t *__restrict__ hit, uint32_t u,
                                                               uint32_t *__restrict__ alive, uint32_t *__restrict__ err) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !alive[i] || hit[i]) return;
    alive[i] = 0u;
    if (u != kNone) atomicMin(err, u);
}

// filter_features: `positions.iter().any(..)` stops at the first position that is unresolved (panic) or overlaps an arm
__global__ __launch_bounds__(kBlock) void plot_stop_kernel(const uint8_t *__restrict__ resolved,
                                                          const uint32_t *__restrict__ hit, uint32_t n_pos,
                                                          uint32_t *__restrict__ stop) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pos) return;
    stop[p] = (!resolved[p] || hit[p]) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void plot_feature_first_kernel(const uint64_t *__restrict__ feat_offs, uint32_t n_feat,
                                                                   const uint8_t *__restrict__ resolved, uint32_t n_pos,
                                                                   const uint32_t *__restrict__ stop,
                                                                   const uint32_t *__restrict__ stop_rank,
                                                                   uint8_t *__restrict__ feat_keep, uint32_t *__restrict__ err) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pos || !stop[p]) return;
    const uint32_t f = segment_of(feat_offs, n_feat, p);
    if (stop_rank[p] != stop_rank[feat_offs[f]]) return;  // a position of this feature stopped the walk before
    if (!resolved[p]) atomicMin(err, p); else feat_keep[f] = 1;
}

__global__ __launch_bounds__(kBlock) void plot_keys_kernel(uint32_t n, const uint32_t *__restrict__ alive,
                                                          const uint32_t *__restrict__ rank, int64_t *__restrict__ keys) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !alive[i]) return;
    keys[rank[i]] = (int64_t)i;
}

__global__ __launch_bounds__(kBlock) void plot_fill_u32_kernel(uint32_t *__restrict__ out, uint32_t n, uint32_t v) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = v;
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_plot {
    std::vector<uint64_t> offs;
    std::vector<int64_t> keys;
    std::vector<uint8_t> feat_keep;
    double ms[3] = {0, 0, 0};
};

namespace {

struct IntervalBuf {
    DevBuf &s, &e, &proper, &owner;
    explicit IntervalBuf(ToolWork &w) : s(w.buf()), e(w.buf()), proper(w.buf()), owner(w.buf()) {}
    int32_t reserve(size_t items) {
        items = std::max<size_t>(items, 2);
        RC_TRY(s.reserve(items * 8));
        RC_TRY(e.reserve(items * 8));
        RC_TRY(proper.reserve(items + 16));
        RC_TRY(owner.reserve(items * 4));
        return 0;
    }
    Intervals view() const { return Intervals{s.as<uint64_t>(), e.as<uint64_t>(), proper.as<uint8_t>(), owner.as<uint32_t>()}; }
};

struct PlotWork : ToolWork {
    DevBuf &offs = buf(), &sds = buf(), &identity = buf(), &feat_offs = buf(), &p_start = buf(), &p_len = buf(), &p_res = buf();
    DevBuf &alive = buf(), &rank = buf(), &matched = buf(), &rank_m = buf(), &hit = buf(), &fam_keep = buf(), &fam_rank = buf(),
           &stop = buf(), &stop_rank = buf(), &feat_keep = buf(), &counters = buf();
    DevBuf &tp_s = buf(), &tp_e = buf(), &ti_s = buf(), &ti_e = buf(), &sorted_s = buf(), &sorted_e = buf();
    IntervalBuf arms{*this}, windows{*this}, improper{*this};
    DevBuf &o_offs = buf(), &o_keys = buf();
    double join_ms = 0;
};

// counters: [0] windows emitted, [1] proper targets, [2] improper targets, [3] improper queries, [4] err of the families /
// duplicons steps, [5] err of the features step
enum { cWindows = 0, cProper = 1, cImproper = 2, cQueries = 3, cErrU = 4, cErrFeat = 5, cCount = 8 };

// hit[owner of q] = 1 for every query that overlaps a target.  cap: the most intervals either list can hold.
int32_t join(PlotWork &w, const Intervals &q, uint32_t nq, const Intervals &t, uint32_t nt, uint32_t force_literal,
             uint32_t *hit) {
    if (!nq || !nt) return 0;
    hipStream_t s = w.s;
    uint32_t *cnt = w.counters.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(cnt + cProper, 0, 12, s));
    RC_TRY(w.tp_s.reserve((size_t)nt * 8));
    RC_TRY(w.tp_e.reserve((size_t)nt * 8));
    RC_TRY(w.ti_s.reserve((size_t)nt * 8));
    RC_TRY(w.ti_e.reserve((size_t)nt * 8));
    plot_split_kernel<<<blocks_for(nt), kBlock, 0, s>>>(t, nt, force_literal, w.tp_s.as<uint64_t>(), w.tp_e.as<uint64_t>(),
                                                        w.ti_s.as<uint64_t>(), w.ti_e.as<uint64_t>(), cnt + cProper);
    HIP_TRY(hipGetLastError());
    uint32_t h[2] = {0, 0};
    HIP_TRY(read_back(h, cnt + cProper, 8, s));
    const uint32_t n_proper = h[0], n_improper = h[1];
    if (n_proper + n_improper != nt) {
        set_error("asgart_plot_filter: %u targets split into %u + %u", nt, n_proper, n_improper);
        return ASGART_E_HIP;
    }
    if (n_improper) {  // every query against the improper targets
        plot_literal_kernel<<<blocks_for(nq), kBlock, 0, s>>>(q.s, q.e, q.owner, nq, w.ti_s.as<uint64_t>(),
                                                              w.ti_e.as<uint64_t>(), n_improper, hit);
        HIP_TRY(hipGetLastError());
    }
    if (!n_proper) return 0;
    RC_TRY(w.sorted_s.reserve((size_t)n_proper * 8));
    RC_TRY(w.sorted_e.reserve((size_t)n_proper * 8));
    RC_TRY(w.sort_keys(w.tp_s.as<uint64_t>(), w.sorted_s.as<uint64_t>(), n_proper));
    RC_TRY(w.sort_keys(w.tp_e.as<uint64_t>(), w.sorted_e.as<uint64_t>(), n_proper));
    RC_TRY(w.improper.reserve(nq));
    const Intervals qi = w.improper.view();
    plot_bisect_kernel<<<blocks_for(nq), kBlock, 0, s>>>(q, nq, w.sorted_s.as<uint64_t>(), w.sorted_e.as<uint64_t>(), n_proper,
                                                         hit, qi, cnt + cQueries);
    HIP_TRY(hipGetLastError());
    uint32_t n_qi = 0;
    HIP_TRY(read_back(&n_qi, cnt + cQueries, 4, s));
    if (n_qi > nq) {
        set_error("asgart_plot_filter: %u improper queries of %u", n_qi, nq);
        return ASGART_E_HIP;
    }
    if (n_qi) {  // the improper queries against the proper targets
        plot_literal_kernel<<<blocks_for(n_qi), kBlock, 0, s>>>(qi.s, qi.e, qi.owner, n_qi, w.tp_s.as<uint64_t>(),
                                                                w.tp_e.as<uint64_t>(), n_proper, hit);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int32_t check_arguments(const uint64_t *fam_offsets, int64_t n_families, const asgart_proto_sd *sds, const float *identity,
                        int64_t n_sd, const uint64_t *feat_offsets, int64_t n_features, const uint64_t *pos_start,
                        const uint64_t *pos_length, const uint8_t *pos_resolved, int64_t n_positions,
                        const asgart_plot_options *opt, asgart_plot **out) {
    if (!out || !fam_offsets || !feat_offsets || !opt || n_families < 0 || n_sd < 0 || n_features < 0 || n_positions < 0 ||
        (n_sd && (!sds || !identity)) || (n_positions && (!pos_start || !pos_length || !pos_resolved))) {
        set_error("asgart_plot_filter: bad argument");
        return ASGART_E_ARG;
    }
    const int64_t cap = ((int64_t)1 << 30) - 1;  // two arms per duplication in one 32-bit list
    if (n_sd >= cap || n_families >= cap || n_features >= cap || n_positions >= cap) {
        set_error("asgart_plot_filter: 2^30 duplications, families, features or positions and more are not supported");
        return ASGART_E_CAP;
    }
    RC_TRY(check_csr("asgart_plot_filter", "fam_offsets", fam_offsets, n_families, n_sd, "n_sd", "entry"));
    return check_csr("asgart_plot_filter", "feat_offsets", feat_offsets, n_features, n_positions, "n_positions", "entry");
}

int32_t run_plot(PlotWork &w, asgart_plot *res, const uint64_t *fam_offsets, uint32_t nf, const asgart_proto_sd *sds,
                 const float *identity, uint32_t n, const uint64_t *feat_offsets, uint32_t n_feat, const uint64_t *pos_start,
                 const uint64_t *pos_length, const uint8_t *pos_resolved, uint32_t n_pos, const asgart_plot_options &opt,
                 int64_t *err_position) {
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t u = kNone;  // the first unresolved position
    for (uint32_t p = 0; p < n_pos; ++p)
        if (!pos_resolved[p]) {
            u = p;
            break;
        }
    const uint32_t before_u = u == kNone ? n_pos : u;
    RC_TRY(w.open(4));
    hipStream_t s = w.s;
    RC_TRY(w.upload(w.offs, fam_offsets, ((size_t)nf + 1) * 8));
    RC_TRY(w.upload(w.sds, sds, (size_t)n * sizeof(asgart_proto_sd)));
    RC_TRY(w.upload(w.identity, identity, (size_t)n * 4));
    RC_TRY(w.upload(w.feat_offs, feat_offsets, ((size_t)n_feat + 1) * 8));
    RC_TRY(w.upload(w.p_start, pos_start, (size_t)n_pos * 8));
    RC_TRY(w.upload(w.p_len, pos_length, (size_t)n_pos * 8));
    RC_TRY(w.upload(w.p_res, pos_resolved, n_pos));
    // every flag array carries one closing zero, so that an exclusive scan over items + 1 ends in the total
    RC_TRY(w.alive.reserve(((size_t)n + 1) * 4));
    RC_TRY(w.rank.reserve(((size_t)n + 1) * 4));
    RC_TRY(w.matched.reserve(((size_t)n + 1) * 4));
    RC_TRY(w.rank_m.reserve(((size_t)n + 1) * 4));
    RC_TRY(w.hit.reserve(((size_t)std::max(n, n_pos) + 1) * 4));
    RC_TRY(w.fam_keep.reserve(((size_t)nf + 1) * 4));
    RC_TRY(w.fam_rank.reserve(((size_t)nf + 1) * 4));
    RC_TRY(w.stop.reserve(((size_t)n_pos + 1) * 4));
    RC_TRY(w.stop_rank.reserve(((size_t)n_pos + 1) * 4));
    RC_TRY(w.feat_keep.reserve((size_t)n_feat + 16));
    RC_TRY(w.counters.reserve(cCount * 4));
    RC_TRY(w.arms.reserve(2 * (size_t)n));
    RC_TRY(w.windows.reserve(n_pos));
    uint32_t *alive = w.alive.as<uint32_t>(), *rank = w.rank.as<uint32_t>(), *matched = w.matched.as<uint32_t>(),
             *rank_m = w.rank_m.as<uint32_t>(), *hit = w.hit.as<uint32_t>(), *fam_keep = w.fam_keep.as<uint32_t>(),
             *fam_rank = w.fam_rank.as<uint32_t>(), *stop = w.stop.as<uint32_t>(), *stop_rank = w.stop_rank.as<uint32_t>(),
             *cnt = w.counters.as<uint32_t>();
    uint8_t *feat_keep = w.feat_keep.as<uint8_t>();
    const uint64_t *d_offs = w.offs.as<uint64_t>(), *d_feat_offs = w.feat_offs.as<uint64_t>();
    const asgart_proto_sd *d_sds = w.sds.as<asgart_proto_sd>();
    const uint8_t *d_res = w.p_res.as<uint8_t>();
    const Intervals arms = w.arms.view(), windows = w.windows.view();
    HIP_TRY(hipMemsetAsync(alive + n, 0, 4, s));
    HIP_TRY(hipMemsetAsync(matched + n, 0, 4, s));
    HIP_TRY(hipMemsetAsync(fam_keep + nf, 0, 4, s));
    HIP_TRY(hipMemsetAsync(stop + n_pos, 0, 4, s));
    HIP_TRY(hipMemsetAsync(cnt, 0, cCount * 4, s));
    HIP_TRY(hipMemsetAsync(cnt + cErrU, 0xFF, 8, s));
    HIP_TRY(hipEventRecord(w.ev[0], s));
    if (n) {
        plot_flags_kernel<<<blocks_for(n), kBlock, 0, s>>>(d_sds, w.identity.as<float>(), n, opt, alive);
        HIP_TRY(hipGetLastError());
    }
    if (nf) {
        plot_fill_u32_kernel<<<blocks_for(nf), kBlock, 0, s>>>(fam_keep, nf, 1u);
        HIP_TRY(hipGetLastError());
    }
    uint32_t n_alive = 0;
    // rank of every duplication alive, and their arms as a list
    auto rescan = [&](bool with_arms) -> int32_t {
        RC_TRY(w.exclusive_scan(alive, rank, (size_t)n + 1));
        HIP_TRY(read_back(&n_alive, rank + n, 4, s));
        if (n_alive > n) {
            set_error("asgart_plot_filter: %u of %u duplications alive", n_alive, n);
            return ASGART_E_HIP;
        }
        if (with_arms && n_alive) {
            plot_emit_arms_kernel<<<blocks_for(n), kBlock, 0, s>>>(d_sds, n, alive, rank, arms);
            HIP_TRY(hipGetLastError());
        }
        return 0;
    };
    // the windows of the resolved positions in [0, limit) under threshold t -> their number
    auto emit_windows = [&](uint32_t limit, uint64_t t, uint32_t *n_windows) -> int32_t {
        *n_windows = 0;
        if (!limit) return 0;
        HIP_TRY(hipMemsetAsync(cnt + cWindows, 0, 4, s));
        plot_emit_windows_kernel<<<blocks_for(limit), kBlock, 0, s>>>(w.p_start.as<uint64_t>(), w.p_len.as<uint64_t>(), d_res,
                                                                     limit, t, windows, cnt + cWindows);
        HIP_TRY(hipGetLastError());
        HIP_TRY(read_back(n_windows, cnt + cWindows, 4, s));
        if (*n_windows > limit) {
            set_error("asgart_plot_filter: %u windows of %u positions", *n_windows, limit);
            return ASGART_E_HIP;
        }
        return 0;
    };
    auto timed_join = [&](const Intervals &q, uint32_t nq, const Intervals &t, uint32_t nt, uint32_t *h) -> int32_t {
        HIP_TRY(hipEventRecord(w.ev[2], s));
        RC_TRY(join(w, q, nq, t, nt, opt.force_literal, h));
        HIP_TRY(hipEventRecord(w.ev[3], s));
        HIP_TRY(stream_sync(s));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, w.ev[2], w.ev[3]));
        w.join_ms += (double)ms;
        return 0;
    };
    // the reference's panic in filter_families / filter_duplicons: always at U
    auto check_u = [&]() -> int32_t {
        uint32_t e = kNone;
        HIP_TRY(read_back(&e, cnt + cErrU, 4, s));
        if (e == kNone) return 0;
        *err_position = (int64_t)e;
        set_error("asgart_plot_filter: position %u is on a fragment the map does not hold and a duplication reaches it "
                  "(the reference panics there, src/bin/asgart-plot.rs:47-50 / :96-99)", e);
        return ASGART_E_ARG;
    };
    const bool any_join = opt.filter_families || opt.filter_duplicons || opt.filter_features;
    RC_TRY(rescan(any_join));
    uint32_t n_windows = 0;
    if (opt.filter_families) {
        RC_TRY(emit_windows(before_u, opt.families_threshold, &n_windows));
        HIP_TRY(hipMemsetAsync(hit, 0, ((size_t)n + 1) * 4, s));
        RC_TRY(timed_join(arms, 2 * n_alive, windows, n_windows, hit));
        if (n) {
            plot_family_first_kernel<<<blocks_for(n), kBlock, 0, s>>>(d_offs, nf, n, alive, rank, hit, u, matched, cnt + cErrU);
            HIP_TRY(hipGetLastError());
        }
        RC_TRY(w.exclusive_scan(matched, rank_m, (size_t)n + 1));
        if (nf) {
            plot_family_keep_kernel<<<blocks_for(nf), kBlock, 0, s>>>(d_offs, nf, rank, rank_m, u, fam_keep);
            HIP_TRY(hipGetLastError());
        }
        if (n) {
            plot_family_apply_kernel<<<blocks_for(n), kBlock, 0, s>>>(d_offs, nf, n, fam_keep, alive);
            HIP_TRY(hipGetLastError());
        }
        RC_TRY(check_u());
        RC_TRY(rescan(opt.filter_duplicons || opt.filter_features));
    }
    if (opt.filter_duplicons) {
        RC_TRY(emit_windows(before_u, opt.duplicons_threshold, &n_windows));
        HIP_TRY(hipMemsetAsync(hit, 0, ((size_t)n + 1) * 4, s));
        RC_TRY(timed_join(arms, 2 * n_alive, windows, n_windows, hit));
        if (n) {
            plot_duplicons_kernel<<<blocks_for(n), kBlock, 0, s>>>(n, hit, u, alive, cnt + cErrU);
            HIP_TRY(hipGetLastError());
        }
        RC_TRY(check_u());
        RC_TRY(rescan(opt.filter_features));
    }
    HIP_TRY(hipMemsetAsync(feat_keep, opt.filter_features ? 0 : 1, (size_t)n_feat + 16, s));
    if (opt.filter_features && n_pos) {
        RC_TRY(emit_windows(n_pos, opt.features_threshold, &n_windows));
        HIP_TRY(hipMemsetAsync(hit, 0, ((size_t)n_pos + 1) * 4, s));
        RC_TRY(timed_join(windows, n_windows, arms, 2 * n_alive, hit));
        plot_stop_kernel<<<blocks_for(n_pos), kBlock, 0, s>>>(d_res, hit, n_pos, stop);
        HIP_TRY(hipGetLastError());
        RC_TRY(w.exclusive_scan(stop, stop_rank, (size_t)n_pos + 1));
        plot_feature_first_kernel<<<blocks_for(n_pos), kBlock, 0, s>>>(d_feat_offs, n_feat, d_res, n_pos, stop, stop_rank,
                                                                      feat_keep, cnt + cErrFeat);
        HIP_TRY(hipGetLastError());
        uint32_t e = kNone;
        HIP_TRY(read_back(&e, cnt + cErrFeat, 4, s));
        if (e != kNone) {
            *err_position = (int64_t)e;
            set_error("asgart_plot_filter: position %u is on a fragment the map does not hold and no position of its "
                      "feature before it overlaps a duplication (the reference panics there, src/bin/asgart-plot.rs:142-145)", e);
            return ASGART_E_ARG;
        }
    }
    RC_TRY(w.exclusive_scan(fam_keep, fam_rank, (size_t)nf + 1));
    uint32_t nf_out = 0;
    HIP_TRY(read_back(&nf_out, fam_rank + nf, 4, s));
    if (nf_out > nf) {
        set_error("asgart_plot_filter: %u of %u families kept", nf_out, nf);
        return ASGART_E_HIP;
    }
    RC_TRY(w.o_offs.reserve(((size_t)nf_out + 1) * 8));
    RC_TRY(w.o_keys.reserve(std::max<size_t>((size_t)n_alive * 8, 16)));
    family_offsets_kernel<kBlock><<<blocks_for((uint64_t)nf + 1), kBlock, 0, s>>>(d_offs, nf, n, rank, fam_keep, fam_rank,
                                                                                 w.o_offs.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    if (n) {
        plot_keys_kernel<<<blocks_for(n), kBlock, 0, s>>>(n, alive, rank, w.o_keys.as<int64_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(w.ev[1], s));
    res->offs.resize((size_t)nf_out + 1);
    res->keys.resize(n_alive);
    res->feat_keep.resize(n_feat);
    HIP_TRY(stream_sync(s));
    HIP_TRY(hipMemcpyAsync(res->offs.data(), w.o_offs.p, ((size_t)nf_out + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n_alive) HIP_TRY(hipMemcpyAsync(res->keys.data(), w.o_keys.p, (size_t)n_alive * 8, hipMemcpyDeviceToHost, s));
    if (n_feat) HIP_TRY(hipMemcpyAsync(res->feat_keep.data(), feat_keep, n_feat, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_sync(s));
    float a = 0;
    HIP_TRY(hipEventElapsedTime(&a, w.ev[0], w.ev[1]));
    res->ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    res->ms[1] = (double)a;
    res->ms[2] = w.join_ms;
    return 0;
}

}  // namespace

extern "C" int32_t asgart_plot_filter(int32_t device, const uint64_t *fam_offsets, int64_t n_families,
                                      const asgart_proto_sd *sds, const float *identity, int64_t n_sd,
                                      const uint64_t *feat_offsets, int64_t n_features, const uint64_t *pos_start,
                                      const uint64_t *pos_length, const uint8_t *pos_resolved, int64_t n_positions,
                                      const asgart_plot_options *options, int64_t *err_position, asgart_plot **out) {
    if (out) *out = nullptr;
    if (err_position) *err_position = -1;
    RC_TRY(check_arguments(fam_offsets, n_families, sds, identity, n_sd, feat_offsets, n_features, pos_start, pos_length,
                           pos_resolved, n_positions, options, out));
    RC_TRY(use_device("asgart_plot_filter", device));
    int64_t err_pos = -1;
    const int32_t rc = run_tool<PlotWork>(out, [&](PlotWork &w, asgart_plot *res) {
        return run_plot(w, res, fam_offsets, (uint32_t)n_families, sds, identity, (uint32_t)n_sd, feat_offsets,
                        (uint32_t)n_features, pos_start, pos_length, pos_resolved, (uint32_t)n_positions, *options, &err_pos);
    });
    if (err_position) *err_position = err_pos;
    return rc;
}

extern "C" void asgart_plot_counts(const asgart_plot *r, uint64_t *n_families, uint64_t *n_sds, uint64_t *n_features) {
    if (n_families) *n_families = r ? r->offs.size() - 1 : 0;
    if (n_sds) *n_sds = r ? r->keys.size() : 0;
    if (n_features) *n_features = r ? r->feat_keep.size() : 0;
}

extern "C" void asgart_plot_copy(const asgart_plot *r, uint64_t *fam_offsets, int64_t *keys, uint8_t *feature_keep) {
    if (!r) return;
    if (fam_offsets) memcpy(fam_offsets, r->offs.data(), r->offs.size() * 8);
    if (keys && !r->keys.empty()) memcpy(keys, r->keys.data(), r->keys.size() * 8);
    if (feature_keep && !r->feat_keep.empty()) memcpy(feature_keep, r->feat_keep.data(), r->feat_keep.size());
}

extern "C" int32_t asgart_plot_timings(const asgart_plot *r, double *ms3) {
    return copy_ms3("asgart_plot_timings", r, ms3);
}

extern "C" void asgart_plot_free(asgart_plot *r) { delete r; }

extern "C" void asgart_plot_geometry(uint64_t *block_threads, uint64_t *tile_windows) {
    if (block_threads) *block_threads = kBlock;
    if (tile_windows) *tile_windows = kTile;
}
