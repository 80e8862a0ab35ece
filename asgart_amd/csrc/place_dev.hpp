// place_dev.hpp -- the placement: every segment gets an extension tier and a sort key, or is proved barren and not run.
//
//   PlaceParams, place_tier, placement_key   tier by live-arm bound, hit total and length; the tail rule
//   segment_is_barren                        barren by the number of hit-probes
//   seg_stats_lanes_kernel                   the walk over the hit counts, a segment per lane (up to kLaneWalk probes)
//   seg_stats_kernel                         ... a wave per segment, for the long ones
//   cluster_barren_kernel                    barren by the positions of the hits (a wave per segment)
//   tier_bounds_kernel                       the tiers' list lengths from the sorted keys
#pragma once

#include "device_base.hpp"

namespace asgart {

// ---------------------------------------------------------------- placement ---
// Every live arm was created or extended by a distinct hit of the last t* processed probes, so
// B = max over probes of (hits of this probe + hits of the previous t* processed probes) bounds
// live arms + new arms from above: the tier whose capacity fits B never overflows (the cascade
// serves the tiers that accept segments above their capacity by an allowance, and the test knobs).
// key = (tier-1) << 29 | (2^29-1 - min(total hits, 2^29-1)): ascending sort = tier, longest first.
struct PlaceParams {
    uint32_t cap[kTiers - 1];   // live-arm capacity of tiers 1..kTiers-1 (0: tier unused); the last takes the rest
    uint32_t sum1;              // segments with more hits than this never go to the one-wave tier
    int force_tier;             // tests: minimum tier for segments with a multi-hit probe
    uint32_t long3;             // > 0: tier 3 is reserved for segments of at least this many probes
    uint32_t long3_big;         // ... or this many, for segments beyond tier 5's capacity
    uint32_t dense6;            // > 0: segments bound for tier 6 by their arms go to tier 3 (when they fit it) with at least this
                                // many hits per processed probe: the dense ones of ANY length on the kernel with a control wave
    uint32_t stats;             // 1 (option debug): hit-probes and hits per tier are tallied (one atomic pair per segment)
    uint32_t barren;            // 1: segments that provably emit nothing are not run at all (segment_is_barren)
    uint2 *seg_info;            // per segment, for cluster_barren_kernel: x = hits, y = probe positions walked | bit 31: the walk saw the
                                // segment's end (not cut short by a sharded call's window); null: not recorded
    uint32_t k, step, G;        // (of the call: for that bound)
    unsigned long long M;
    uint32_t dense3;            // > 0: ... and only the DENSE ones (at least this many hits per processed probe on average:
                                // tandem arrays); the sparse long ones (a chromosome against its homologue: a few hits per
                                // probe, mostly run by one wave alone) go to tier 6's kernel -- set when tier 3 runs the
                                // kernel with a control wave, whose step costs the same whatever the probe holds
    uint32_t tail_hits[kTiers - 1];  // tail_hits[t - 1] > 0 (tiers 2, 4, 5): a segment its arm bound sends to tier t goes, with at least this
                                // many hits, to the next tier that holds more instead (the tail rule, place_tier); 0: tier t keeps its own
};

// A segment that cannot emit anything need not run.  A family holds the arms whose RIGHT segment is at least M long
// (src/automaton.rs:186-196), and a right segment only grows when its arm is extended (:136-143): to m.end = x + k with
// x < right.end + threshold (:68-70), i.e. by at most threshold + k - 1 per extension, at most once per hit-probe.  With
// H hit-probes in the segment an arm born at the first is extended at most H - 1 times, and its threshold
// max(G, len(left) / 10) is at most max(G, (span * step + k) / 10) while the segment spans `span` probe positions
// (len(left) = i + k - left.start <= span * step + k).  So
//     k + (H - 1) * (thr_max + k - 1) < M   =>   no arm of the segment ever reaches M: it emits no family, and -- segments being
// independent automaton instances -- leaving it out changes nothing.  At the defaults (k = 20, G = 120,
// M = 1000) that is every segment of up to 8 hit-probes: most of the million-odd tiny segments of a genome-sized pass.
// (Not when the walk was cut short by the end of a sharded call's window: the segment may go on beyond it.)
constexpr int kTierBarren = kTiers + 1;
__device__ inline bool segment_is_barren(const PlaceParams &pp, uint32_t n_hit, uint32_t span_probes) {
    if (!pp.barren || n_hit == 0u) return false;
    const unsigned long long len_left_max = (unsigned long long)span_probes * pp.step + pp.k;
    const unsigned long long thr_max = max((unsigned long long)pp.G, len_left_max / 10ull);
    return (unsigned long long)pp.k + (unsigned long long)(n_hit - 1u) * (thr_max + pp.k - 1ull) < pp.M;
}

// Sort key of a segment inside its tier (ascending = launch order).  Heavy tiers: longest first,
// so that the serial chains start early.  Tier 1 holds over a million mostly tiny segments whose
// cost is the latency of fetching their probe rows: apart from its few long ones (first, by
// length) they run in genome order, so that the segments in flight at any time share cache lines
// and pages of p_filt / row_off / hits.
__device__ inline uint32_t placement_key(int tier, unsigned long long sum, uint32_t g0) {
    uint32_t low;
    if (tier == 1) {
        low = sum >= 1024ull ? 1023u - (uint32_t)min(sum >> 5, 1023ull) : 1024u + (g0 >> 4);
    } else {
        const uint32_t s29 = sum > 0x1FFFFFFFull ? 0x1FFFFFFFu : (uint32_t)sum;
        low = 0x1FFFFFFFu - s29;
    }
    return (((uint32_t)tier - 1u) << 29) | low;
}

// The next tier above src that is in use and holds more arms than src (cap[t - 1]: tier t's capacity, 0: not in use; tier
// kTiers takes whatever is left); tier `skip` is passed over.  Where the cascade re-runs what src gave up on (skip = 0), and
// where the tail rule sends a long segment (skip = 3).
__host__ __device__ inline int next_holding_more(const uint32_t *cap, int src, int skip = 0) {
    int dst = src + 1;
    while (dst < kTiers && (dst == skip || cap[dst - 1] == 0u || cap[dst - 1] <= cap[src - 1])) ++dst;
    return dst;
}

// Tier of a segment from its live-arm bound, hit total and processed-probe count.  With long3 set,
// tier 3 (lowest per-probe latency, one workgroup of 1024 threads per CU) only takes the long
// segments whose serial chain is the critical path of a pass; everything else goes by capacity.
// The tail rule: a launch lasts as long as its longest segment, and a stream that carries two launches (a call has fewer
// hardware queues than tiers) runs the second one's longest segment behind the first one's.  The few segments that make up
// the tail of a thresholded tier -- those with tail_hits hits and more -- go to the next arm-resident workgroup tier (4, 5,
// 6) that holds more, whose launch a longer segment bounds anyway.  More capacity is always safe; tier 3 is never entered
// this way (long3 / dense3 / dense6 decide that, above and below).  *tail_up: the rule moved the segment.
__device__ inline int place_tier(uint32_t bound, unsigned long long sum, uint32_t n_probes, const PlaceParams &pp, bool *tail_up) {
    *tail_up = false;
    if (bound <= pp.cap[0] && sum <= pp.sum1) return 1;
    // tier 6 pays ~3x tier 3's time per probe (many arms per thread): its segments count as long
    // from a quarter of the threshold on
    if (pp.long3 && bound <= pp.cap[2] &&
        (n_probes >= pp.long3 || (bound > pp.cap[4] && n_probes >= pp.long3_big))) {
        if (!pp.dense3 || sum >= (unsigned long long)pp.dense3 * n_probes || bound > pp.cap[5]) return 3;
        return 6;  // (the long segments that are not dense: mostly run by one wave alone, on K6's solo probes)
    }
    for (int t = 2; t < kTiers; ++t) {
        if (t == 3 && pp.long3) continue;
        if (bound <= pp.cap[t - 1]) {
            if (t == 6 && pp.dense6 && bound <= pp.cap[2] && sum >= (unsigned long long)pp.dense6 * n_probes) return 3;
            if (pp.tail_hits[t - 1] && sum >= (unsigned long long)pp.tail_hits[t - 1]) {
                const int up = next_holding_more(pp.cap, t, 3);
                if (up >= 4 && up <= 6) {
                    *tail_up = true;
                    return up;
                }
            }
            return t;
        }
    }
    return kTiers;
}

// The placement walk reads the per-probe hit counts only -- no hit accesses at all.
//
// Most segments are a handful of probes long (3.4 M segments per GRCh38-shaped step, a dozen probes each), and a
// wave per segment spends its time on the per-segment chain of dependent loads.  So the first kernel walks ONE
// SEGMENT PER LANE, 64 segments per wave side by side, for at most kLaneWalk probes; the few segments that are
// longer go to a list and the wave-per-segment kernel below (64 probes per round trip) finishes them.
constexpr uint32_t kLaneWalk = 256;

__global__ __launch_bounds__(64) void seg_stats_lanes_kernel(RunParams rp, const uint32_t *__restrict__ p_filt,
                                                             const uint32_t *__restrict__ seg_list,
                                                             const unsigned long long *__restrict__ n_seg_ptr,
                                                             uint32_t *__restrict__ keys,
                                                             uint32_t *__restrict__ vals, PlaceParams pp,
                                                             uint32_t *__restrict__ long_list,
                                                             unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t s_ring[65 * 64];  // [slot][lane]: hit counts of the last TW + 1 processed probes
    const uint32_t lane = threadIdx.x;
    const uint64_t n_seg = *n_seg_ptr;
    const uint32_t RW = min(rp.tstar, 64u) + 1u;
    for (uint64_t base = (uint64_t)blockIdx.x * 64u; base < n_seg; base += (uint64_t)gridDim.x * 64u) {
        const uint64_t sidx = base + lane;
        const bool have = sidx < n_seg;
        uint32_t g0 = 0, g_end = 0;
        bool window_cut = false;  // the walk may end at the end of a sharded call's window instead of the chunk's
        if (have) {
            g0 = seg_list[sidx];
            const uint32_t chunk_end = rp.ch.pbase[chunk_of(rp.ch, g0) + 1];
            g_end = min(chunk_end, rp.win_end(g0));
            window_cut = g_end < chunk_end;
        }
        for (uint32_t r = 0; r < RW; ++r) s_ring[r * 64u + lane] = 0;
        uint32_t quiet = 0, mx = 0, bound = 0, n_probes = 0, wsum = 0, head = 0, steps = 0, g = g0, n_hit = 0;
        unsigned long long sum = 0;
        bool done = !have, by_quiet = false;
        while (!done && g < g_end && steps < kLaneWalk) {
            const uint32_t f = p_filt[g];
            ++g;
            ++steps;
            const bool hit = f >= 1u && f < kPending;
            if (!hit && f != 0u) continue;  // skipped probes (N, cardinality) are not processed
            if (!hit) {
                if (++quiet >= rp.tstar) {  // t* quiet probes: every arm has been retired, the segment is over
                    done = true;
                    by_quiet = true;
                    break;
                }
            } else {
                quiet = 0;
            }
            const uint32_t v = hit ? f : 0u;
            ++n_probes;
            n_hit += hit ? 1u : 0u;
            const uint32_t at = head * 64u + lane;
            wsum += v - s_ring[at];
            s_ring[at] = v;
            head = head + 1u == RW ? 0u : head + 1u;
            bound = max(bound, wsum);
            mx = max(mx, v);
            sum += v;
        }
        if (g >= g_end) done = true;
        if (have && done) {
            if (rp.tstar > 64u) bound = 0xFFFFFFFFu;  // no estimate for huge gap settings: largest tier
            bool tail_up;
            int tier = place_tier(bound, sum, n_probes, pp, &tail_up);
            if (mx > 1 && pp.force_tier > tier) tier = min(pp.force_tier, kTiers);
            if ((by_quiet || !window_cut) && segment_is_barren(pp, n_hit, g - g0)) tier = kTierBarren;
            if (tail_up && tier != kTierBarren) atomicAdd(&ctr[CT_TAIL_UP], 1ull);
            keys[sidx] = placement_key(tier, sum, g0);
            vals[sidx] = g0;
            if (pp.seg_info)
                pp.seg_info[sidx] = make_uint2(sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum,
                                               (g - g0) | ((by_quiet || !window_cut) ? 0x80000000u : 0u));
            if (pp.stats) {
                atomicAdd(&ctr[CT_TPROBES1 + tier - 1], (unsigned long long)n_hit);
                atomicAdd(&ctr[CT_THITS1 + tier - 1], sum);
            }
        }
        const unsigned long long lm = __ballot(have && !done);
        if (lm) {
            const int leader = __ffsll((long long)lm) - 1;
            unsigned long long at = 0;
            if ((int)lane == leader) at = atomicAdd(&ctr[CT_LONGSEG], (unsigned long long)__popcll(lm));
            at = __shfl(at, leader);
            if (have && !done) long_list[at + __popcll(lm & ((1ull << lane) - 1ull))] = (uint32_t)sidx;
        }
    }
}

// One wave per segment: the entries idx_list[0 .. *n_ptr) of the segment list (all of it when idx_list is null).
__global__ __launch_bounds__(64) void seg_stats_kernel(RunParams rp, const uint32_t *__restrict__ p_filt,
                                                       const uint32_t *__restrict__ seg_list,
                                                       const unsigned long long *__restrict__ n_ptr,
                                                       const uint32_t *__restrict__ idx_list,
                                                       uint32_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals, PlaceParams pp,
                                                       unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t s_ext[64 + 64];  // [0,TW): hit counts of the previous processed probes
    const int lane = threadIdx.x;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint64_t n_items = *n_ptr;
    const uint32_t TW = min(rp.tstar, 64u);
    for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint64_t sidx = idx_list ? (uint64_t)idx_list[item] : item;
        const uint32_t g0 = seg_list[sidx];
        const int c = chunk_of_uniform(rp.ch, g0);
        const uint32_t g_end = min(rp.ch.pbase[c + 1], rp.win_end(g0));
        const bool window_cut = g_end < rp.ch.pbase[c + 1];
        uint32_t quiet = 0, mx = 0, bound = 0, n_probes = 0, n_hit = 0, g_stop = g_end, g_after_hit = g0 + 1u;
        unsigned long long sum = 0;
        bool done = false;
        s_ext[lane] = 0;
        lds_barrier();
        // the next batch's hit counts are in flight while this one is processed: a long segment's walk is a chain
        // of dependent round trips (64 probes each) and sets the duration of the whole launch
        uint32_t f_next = g0 + (uint32_t)lane < g_end ? p_filt[g0 + lane] : kSkipN;
        for (uint32_t g = g0; g < g_end && !done; g += 64) {
            const uint32_t f = f_next;
            f_next = g + 64u + (uint32_t)lane < g_end ? p_filt[g + 64u + lane] : kSkipN;
            const unsigned long long hm = __ballot(f >= 1u && f < kPending);
            const unsigned long long qm = __ballot(f == 0u);
            if (!(hm | qm)) continue;  // 64 skipped probes (cardinality, N): nothing is processed, nothing changes
            unsigned long long live = ~0ull;  // probes of this batch that belong to the segment
            // The segment ends with the t*-th quiet probe in a row (skipped probes neither count nor interrupt,
            // a hit restarts the count).  Every lane prices the quiet run that ends at its own probe -- no walk
            // from hit to hit: in a dense array with interleaved quiet probes that scalar walk, 40-odd dependent
            // steps per batch, was the whole cost of placing the longest segment.
            {
                const unsigned long long hb = hm & lt_mask;  // hits before this lane
                const int lh = hb ? 63 - __clzll((long long)hb) : -1;
                const unsigned long long above_lh = lh < 0 ? ~0ull : (lh == 63 ? 0ull : ~((2ull << lh) - 1ull));
                const uint32_t run = (uint32_t)__popcll(qm & (lt_mask | (1ull << lane)) & above_lh) + (lh < 0 ? quiet : 0u);
                const unsigned long long term = __ballot(((qm >> lane) & 1ull) && run >= rp.tstar);
                if (term) {
                    // the run that reaches t* starts behind the hit at lh (of the terminating lane): only the
                    // probes up to that hit still belong to the segment
                    const uint32_t pos = (uint32_t)(__shfl(lh, __ffsll((long long)term) - 1) + 1);
                    done = true;
                    // (exactly behind the segment's last hit-probe: the barren tests want an upper bound of the span, the
                    // cutting into ranges must never place a cut on a hit-probe of the NEXT segment)
                    g_stop = pos ? g + pos : g_after_hit;
                    live = (1ull << pos) - 1ull;  // pos <= 63
                } else {
                    const int last = hm ? 63 - __clzll((long long)hm) : -1;
                    if (last >= 0) g_after_hit = g + (uint32_t)last + 1u;
                    const unsigned long long above = last < 0 ? ~0ull : (last == 63 ? 0ull : ~((2ull << last) - 1ull));
                    quiet = (uint32_t)__popcll(qm & above) + (last < 0 ? quiet : 0u);
                }
            }
            const unsigned long long procm = (hm | qm) & live;
            const bool proc = (procm >> lane) & 1ull;
            const uint32_t v = ((hm & live) >> lane) & 1ull ? f : 0u;
            const uint32_t r = (uint32_t)__popcll(procm & lt_mask);
            const uint32_t n_proc = (uint32_t)__popcll(procm);
            n_probes += n_proc;
            n_hit += (uint32_t)__popcll(hm & live);
            if (proc) s_ext[TW + r] = v;
            lds_barrier();
            uint32_t wsum = 0;
            if (proc)
                for (uint32_t d = 0; d <= TW; ++d) wsum += s_ext[TW + r - d];
            uint32_t m = v, wm = wsum;
            unsigned long long sv = v;
            for (int off = 32; off > 0; off >>= 1) {
                sv += __shfl_down(sv, off);
                m = max(m, (uint32_t)__shfl_down(m, off));
                wm = max(wm, (uint32_t)__shfl_down(wm, off));
            }
            sum += __shfl(sv, 0);
            mx = max(mx, (uint32_t)__shfl(m, 0));
            bound = max(bound, (uint32_t)__shfl(wm, 0));
            const uint32_t keep = (uint32_t)lane < TW ? s_ext[n_proc + lane] : 0u;
            lds_barrier();
            if ((uint32_t)lane < TW) s_ext[lane] = keep;
            lds_barrier();
        }
        if (rp.tstar > 64u) bound = 0xFFFFFFFFu;
        if (lane == 0) {
            bool tail_up;
            int tier = place_tier(bound, sum, n_probes, pp, &tail_up);
            if (mx > 1 && pp.force_tier > tier) tier = min(pp.force_tier, kTiers);
            if ((done || !window_cut) && segment_is_barren(pp, n_hit, min(g_stop, g_end) - g0)) tier = kTierBarren;
            if (tail_up && tier != kTierBarren) atomicAdd(&ctr[CT_TAIL_UP], 1ull);
            keys[sidx] = placement_key(tier, sum, g0);
            vals[sidx] = g0;
            if (pp.seg_info)
                pp.seg_info[sidx] = make_uint2(sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum,
                                               (min(g_stop, g_end) - g0) | ((done || !window_cut) ? 0x80000000u : 0u));
            if (pp.stats) {
                atomicAdd(&ctr[CT_TPROBES1 + tier - 1], (unsigned long long)n_hit);
                atomicAdd(&ctr[CT_THITS1 + tier - 1], sum);
            }
        }
        lds_barrier();
    }
}

// Barren by POSITION.  An arm's right segment is built from a chain of hits x_0 < x_1 < ... (one per hit-probe at most) with
// x_{j+1} < x_j + k + threshold (src/automaton.rs:68-70 with right.end = x_j + k), and it is reported only when
// x_m + k - x_0 >= M.  With buckets of w = k + thr_max positions (thr_max: the largest threshold any arm of the segment can
// have, as in segment_is_barren) every link of a chain stays in its bucket or moves to the next one, so an arm that reaches M
// leaves a RUN of at least floor((M - k) / w) + 1 consecutive occupied buckets among the segment's hits.  No such run =>
// the segment emits nothing.  That is the fate of the bursts of interspersed repeats, which are most of the extension's
// work at genome scale: a probe inside a repeat hits a hundred other copies, every copy collects a few hundred bases of
// hits over the few dozen probes of the burst, the copies are kilobases apart -- hundreds of arms per probe and not one
// duplication.  Tandem arrays and real duplications keep their runs and are run as before.
// One WAVE per segment: the hits' buckets set bits of a hashed LDS bitmap (BITS bits; a collision can only make a bucket look
// occupied that is not, i.e. a run look longer -- the test stays sound, it only proves a little less), then every hit
// asks whether the need - 1 buckets behind its own are all occupied.  Order-free, no barrier between waves, a few KB of
// LDS per wave (the continuation filter of round 2 answered a related question probe by probe, a wave per segment with
// barriers per probe, and cost more than it saved).  Segments of more than max_hits hits are left alone.
template <class PosT, int BITS>
__global__ __launch_bounds__(64) void cluster_barren_kernel(RunParams rp, PlaceParams pp,
                                                            const unsigned long long *__restrict__ row_off,
                                                            const PosT *__restrict__ hits,
                                                            const uint32_t *__restrict__ seg_list,
                                                            const unsigned long long *__restrict__ n_seg_ptr,
                                                            uint32_t *__restrict__ keys, uint32_t min_hits, uint32_t max_hits,
                                                            unsigned long long *__restrict__ cursor,
                                                            unsigned long long *__restrict__ ctr) {
    static_assert((BITS & (BITS - 1)) == 0 && BITS >= 2048, "bitmap size");
    constexpr uint32_t kWords = BITS / 32, kShift = 32 - __builtin_ctz((unsigned)BITS);
    __shared__ uint32_t s_bits[kWords];
    const uint32_t lane = threadIdx.x;
    const uint64_t n_seg = *n_seg_ptr;
    uint32_t n_barren = 0;
    auto bit_of = [&](uint32_t b) { return (b * 2654435761u) >> kShift; };
    for (;;) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, 64ull);
        base = lane_of(base, 0u);
        if (base >= n_seg) break;
        // the 64 segments of the batch side by side: key, hit total, where its rows are (most are not this launch's: already
        // barren, another size class, cut by a sharded window); the candidates are then walked one after the other, their
        // set-up already in registers
        const uint64_t sj = base + lane;
        bool cand = false;
        uint32_t key_l = 0, span_l = 0;
        unsigned long long lo_l = 0, hi_l = 0;
        if (sj < n_seg) {
            key_l = keys[sj];
            const uint2 info = pp.seg_info[sj];
            span_l = info.y & 0x7FFFFFFFu;
            cand = (key_l >> 29) < (uint32_t)kTiers && (info.y >> 31) && info.x >= min_hits && info.x <= max_hits;
            if (cand) {
                const uint32_t g0 = seg_list[sj];
                lo_l = row_off[g0];
                hi_l = row_off[g0 + span_l];
                cand = hi_l > lo_l && hi_l - lo_l <= (unsigned long long)max_hits;
            }
        }
        unsigned long long todo = __ballot(cand);
        while (todo) {
            const uint32_t l = (uint32_t)(__ffsll((long long)todo) - 1);
            todo &= todo - 1ull;
            const uint32_t key = lane_of(key_l, l), span = lane_of(span_l, l);
            const unsigned long long lo = lane_of(lo_l, l);
            const uint32_t n = (uint32_t)(lane_of(hi_l, l) - lo);
            const unsigned long long len_left_max = (unsigned long long)span * pp.step + pp.k;
            const unsigned long long thr_max = max((unsigned long long)pp.G, len_left_max / 10ull);
            const unsigned long long w = thr_max + pp.k;
            const unsigned long long need = (pp.M - pp.k) / w + 1ull;  // consecutive occupied buckets an emitting arm leaves
            if (need < 2ull || need > 64ull) continue;                 // (one bucket proves nothing; M > k: the host has checked)
            // exact floor(x / w) through a double quotient and one correction (x < 2^53; a 64-bit integer division per hit
            // would be a hundred instructions)
            const double inv_w = 1.0 / (double)w;
            auto bucket_of = [&](unsigned long long x) -> uint32_t {
                unsigned long long q = (unsigned long long)((double)x * inv_w);
                const long long r = (long long)(x - q * w);
                q += r >= (long long)w ? 1ull : 0ull;
                q -= r < 0 ? 1ull : 0ull;
                return (uint32_t)q;
            };
            for (uint32_t j = lane; j < kWords; j += 64u) s_bits[j] = 0u;
            __builtin_amdgcn_wave_barrier();
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // (eight independent loads per lane in flight, then the bits: a load-set loop would pay one round trip per pass)
            for (uint32_t j0 = 0; j0 < n; j0 += 512u) {
                PosT xv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    xv[u] = j < n ? hits[lo + j] : (PosT)0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    if (j < n) {
                        const uint32_t bi = bit_of(bucket_of((unsigned long long)xv[u]));
                        atomicOr(&s_bits[bi >> 5], 1u << (bi & 31u));
                    }
                }
            }
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            bool found = false;
            for (uint32_t j0 = 0; j0 < n && !found; j0 += 512u) {
                PosT xv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    xv[u] = j < n ? hits[lo + j] : (PosT)0;
                }
                bool mine = false;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    if (j < n) {
                        const uint32_t b = bucket_of((unsigned long long)xv[u]);
                        bool all = true;
                        for (uint32_t d = 1; d < (uint32_t)need && all; ++d) {
                            const uint32_t bi = bit_of(b + d);
                            all = (s_bits[bi >> 5] >> (bi & 31u)) & 1u;
                        }
                        mine = mine || all;
                    }
                }
                found = __ballot(mine) != 0ull;
            }
            __builtin_amdgcn_wave_barrier();
            if (!found) {
                if (lane == 0) keys[base + l] = (key & 0x1FFFFFFFu) | ((uint32_t)(kTierBarren - 1) << 29);
                ++n_barren;
            }
        }
    }
    if (lane == 0 && n_barren) atomicAdd(&ctr[CT_CLUSTER_BARREN], (unsigned long long)n_barren);
}

// tier list lengths from the sorted placement keys (tier-1 = key >> 29): n_t = first index whose
// tier exceeds t, by bisection -- instead of one contended global atomic per segment
__global__ void tier_bounds_kernel(const uint32_t *__restrict__ sorted_keys,
                                   const unsigned long long *__restrict__ n_seg_ptr,
                                   unsigned long long *__restrict__ ctr) {
    const int t = threadIdx.x;  // 0..4
    if (t >= kTiers) return;
    const uint64_t n = *n_seg_ptr;
    auto first_ge = [&](uint32_t tier_idx) {  // first position with (key >> 29) >= tier_idx
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((sorted_keys[mid] >> 29) < tier_idx) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    ctr[CT_N1 + t] = first_ge((uint32_t)t + 1u) - first_ge((uint32_t)t);
}

}  // namespace asgart
