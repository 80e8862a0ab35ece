// ranges_dev.hpp -- the cut planner of the runs over ranges (option split) and the join of what the runs leave.
//
//   split_tally_kernel, split_pick_kernel   the range length the run budget allows
//   plan_ranges_kernel                      long segments of tiers 3..6 off their lists, cut into runs (RangeRun, SplitSeg:
//                                           extend_common_dev.hpp)
//   top_uncut_kernel                        option debug = 2: the longest segments that were not cut
//   validate_cuts_kernel                    a workgroup per cut: both sides hold the same arms and family state
//   fixup_records_kernel                    family ordinals of the runs' records; records of failed cuts -> void
#pragma once

#include "extend_common_dev.hpp"
#include "place_dev.hpp"

namespace asgart {

// ---- long segments as ranges that run side by side (option split) ---------------------------------------------------------
// The probes of a segment are strictly serial, and the longest segment of a pass is the floor of its extension.  But the arm
// list a tandem array leaves behind at some probe c is, some way into the array, a function of the last few thousand probes
// only: a run that starts with NO arm `warm` probes in front of c holds, at c, exactly the arms (and the family state) of the
// run that started at the segment's first probe -- when it does.  Whether it does is CHECKED, never assumed: the range in
// front of the cut and a warm-up that stops at the cut both write out what they hold there (validate_cuts_kernel compares),
// where a cut fails the ranges in front of it stand, the records of those behind it are dropped and the rest of the segment
// runs as one more run from the last checked state (the whole segment again when its first cut fails).
//   plan_ranges_kernel     one thread per segment: the long ones of the long-shape tiers (3, 6) are taken off their tier's
//                          list and cut at the first hit-probe at or behind every range_len-th probe
//   validate_cuts_kernel   one workgroup per cut: same arms (by creation number, every field), same family state
//   fixup_records_kernel   one thread per record slot: family ordinals of a range + the flushes of the ranges before it;
//                          records of a segment that failed -> void
// Range size by budget (option split_len = 0): every run holds a compute unit, so the number of runs is what the cutting
// may cost.  A segment of `span` probe positions gets round(span / C) ranges of one length.  split_tally_kernel counts, for
// each candidate C, the runs that cutting every eligible segment would make; split_pick_kernel takes the SMALLEST C whose
// count fits the budget (a small job gets small ranges -- its few long segments are its whole extension --, a genome-sized
// one large ranges); warm-up C positions within [2 048, 6 144]; a segment is cut when it is at least 2 C and at least 3
// warm-ups long.  The choice depends on the segments only: the same in every call over the same input and settings.
constexpr int kSplitCand = 12;
__device__ inline uint32_t split_len_of(int c) {
    constexpr uint32_t t[kSplitCand] = {2048, 3072, 4096, 6144, 8192, 12288, 16384, 24576, 32768, 49152, 65536, 98304};
    return t[c];
}
// (half a range was not enough at the middle sizes: with ranges of 6 144 probes -- what a shard of a genome-sized call gets --
// and 3 072 of warm-up 20 of 44 cut segments had a cut that did not hold; with 6 144 every cut of the unsharded call holds)
__device__ inline uint32_t split_warm_of(uint32_t C) { return min(max(C, 2048u), 6144u); }
struct SplitChoice {
    uint32_t range_len, warm, min_span, pad;
    unsigned long long runs[kSplitCand];
};
__device__ inline bool split_eligible(const RunParams &rp, uint32_t key, uint2 info) {
    const uint32_t tier = (key >> 29) + 1u;
    // (tiers 1 and 2 are one-wave kernels: a wave on its own passes a sparse probe several times faster than the long shape's
    // sixteen waves and their barrier -- cutting a yeast-sized input's longest tier-2 segment in two doubled its step; cutting
    // the one-wave segments of 12 288 probe positions and more left a GRCh38-sized step and its shards where they were:
    // DESIGN_HISTORY.md; tier 7's arms do not fit the long shape)
    if (tier < 3u || tier > 6u) return false;
    const uint32_t span = info.y & 0x7FFFFFFFu;
    if (!(info.y >> 31) || span < 128u) return false;  // (cut short by a shard window: left alone)
    // (creation numbers of a run: needle offset relative to the segment's first probe << 10 | hit index)
    return (unsigned long long)span * (unsigned long long)rp.step < (1ull << 22) - 2ull;
}
__global__ __launch_bounds__(256) void split_tally_kernel(RunParams rp, const unsigned long long *__restrict__ n_seg_ptr,
                                                         const uint32_t *__restrict__ keys, const uint2 *__restrict__ seg_info,
                                                         SplitChoice *__restrict__ choice) {
    const unsigned long long sj = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (sj >= *n_seg_ptr) return;
    const uint2 info = seg_info[sj];
    const uint32_t span = info.y & 0x7FFFFFFFu;
    if (span < 3u * 2048u || !split_eligible(rp, keys[sj], info)) return;
    const unsigned long long cost = (unsigned long long)span;
    for (int c = 0; c < kSplitCand; ++c) {
        const unsigned long long C = split_len_of(c);
        if (cost < 2ull * C || span < 3u * split_warm_of((uint32_t)C)) break;
        atomicAdd(&choice->runs[c], max(2ull, (cost + C / 2ull) / C));
    }
}
__global__ void split_pick_kernel(SplitChoice *choice, uint32_t budget) {
    int pick = kSplitCand - 1;
    for (int c = 0; c < kSplitCand; ++c)
        if (choice->runs[c] <= (unsigned long long)budget) {
            pick = c;
            break;
        }
    choice->range_len = split_len_of(pick);
    choice->warm = split_warm_of(split_len_of(pick));  // (E. coli-sized inputs: cuts with 1 024 probes of warm-up did not hold)
    choice->min_span = 3u * choice->warm;               // (two ranges of a shorter segment are each nearly the segment)
}

constexpr uint32_t kSplitBlockedMax = 2048;  // verdicts of earlier calls handed to one call
// what an earlier call of the index found out about a segment a cut of which did not hold
struct BlockedSeg {
    uint32_t g0;         // the segment (first probe, in this call's numbering)
    uint32_t range_len;  // at which range length (the verdict means nothing at another)
    uint32_t allowed;    // how many of its cuts, counted from the segment's start, are planned again (kAllCuts: all of them)
    uint32_t warm;       // the warm-up its ranges get from now on (0: the call's)
};
constexpr uint32_t kAllCuts = 0xFFFFFFFFu;
struct SplitParams {
    uint32_t range_len, warm, min_span;   // size of a range (probe positions; range_len = 0: cost units, as split_pick_kernel chose),
                                          // warm-up probes in front of a cut, shortest segment that is cut
    uint32_t max_runs, max_cuts, max_splits;
    uint32_t n_blocked;
    const BlockedSeg *blocked;            // segments a cut of which did not hold in an earlier call of the index
};
__global__ __launch_bounds__(256) void plan_ranges_kernel(RunParams rp, SplitParams sp, const uint32_t *__restrict__ p_filt,
                                                         const uint32_t *__restrict__ seg_list,
                                                         const unsigned long long *__restrict__ n_seg_ptr,
                                                         uint32_t *__restrict__ keys, const uint2 *__restrict__ seg_info,
                                                         unsigned long long *__restrict__ hdr,  // 0 runs, 1 cuts, 2 split segments
                                                         RangeRun *__restrict__ runs, uint2 *__restrict__ cuts,
                                                         SplitSeg *__restrict__ splits, const SplitChoice *__restrict__ choice) {
    const unsigned long long sj = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (sj >= *n_seg_ptr) return;
    if (!sp.range_len) {  // (hdr[3] is the runs' work cursor: hdr[4] tells the host which length was used)
        sp.range_len = choice->range_len;
        sp.warm = choice->warm;
        sp.min_span = max(sp.min_span, choice->min_span);
        if (sj == 0) hdr[4] = sp.range_len;
    } else if (sj == 0) {
        hdr[4] = sp.range_len;
    }
    const uint32_t key = keys[sj];
    const uint2 info = seg_info[sj];
    const uint32_t span = info.y & 0x7FFFFFFFu;
    if (span < sp.min_span || !split_eligible(rp, key, info)) return;
    const uint32_t g0 = seg_list[sj];
    // a segment a cut of which did not hold in an earlier call: its ranges start as far in front of their cuts as the oldest
    // arm at the failed cut asked for -- or, where that is further than a range is worth, only the cuts that held are planned again
    uint32_t warm = sp.warm;
    uint32_t n_cut_max = 0xFFFFFFFFu;
    for (uint32_t b = 0; b < sp.n_blocked; ++b) {
        const BlockedSeg v = sp.blocked[b];
        if (v.g0 == g0 && v.range_len == sp.range_len) {
            n_cut_max = min(n_cut_max, v.allowed);
            warm = max(warm, v.warm);
        }
    }
    // ranges of about range_len probe positions each, at least two, their cuts at equal shares of the segment; a segment whose
    // cuts held only up to some point in an earlier call keeps those cuts (same places) and runs the rest as its last range
    // (cuts at equal shares of positions + hits / w instead were measured at GRCh38 size and did not move the step: DESIGN_HISTORY.md)
    const unsigned long long total = span, unit = sp.range_len;
    if (total < 2ull * unit) return;
    const uint32_t n_r_all = (uint32_t)min(1024ull, max(2ull, (total + unit / 2ull) / unit));
    const uint32_t n_r = min(n_r_all, n_cut_max == kAllCuts ? n_r_all : n_cut_max + 1u);
    if (n_r < 2u) return;
    auto cut_of = [&](uint32_t j) -> uint32_t {  // first hit-probe at or behind the j-th share of the cost (0: none)
        uint32_t c = g0 + (uint32_t)(total / n_r_all * j);
        while (c < g0 + span) {
            const uint32_t f = p_filt[c];
            if (f >= 1u && f < kPending) return c;
            ++c;
        }
        return 0u;
    };
    {   // (every cut behind its predecessor, the first behind the segment's start)
        uint32_t before = g0;
        for (uint32_t j = 1; j < n_r; ++j) {
            const uint32_t c = cut_of(j);
            if (c <= before) return;
            before = c;
        }
    }
    const uint32_t n_runs = n_r;
    const uint32_t run_base = (uint32_t)atomicAdd(&hdr[0], (unsigned long long)n_runs);
    if (run_base + n_runs > sp.max_runs) {
        atomicAdd(&hdr[0], 0ull - (unsigned long long)n_runs);
        return;
    }
    const uint32_t cut_base = (uint32_t)atomicAdd(&hdr[1], (unsigned long long)(n_r - 1u));
    const uint32_t split = (uint32_t)atomicAdd(&hdr[2], 1ull);
    if (cut_base + n_r - 1u > sp.max_cuts || split >= sp.max_splits) {  // (sized together with max_runs: does not happen)
        atomicAdd(&hdr[0], 0ull - (unsigned long long)n_runs);
        atomicAdd(&hdr[1], 0ull - (unsigned long long)(n_r - 1u));
        atomicAdd(&hdr[2], 0ull - 1ull);
        return;
    }
    keys[sj] = (key & 0x1FFFFFFFu) | ((uint32_t)(kTierBarren - 1) << 29);  // off its tier's list
    splits[split] = SplitSeg{g0, run_base, n_r, cut_base, span, info.x, (key >> 29) + 1u, warm};
    uint32_t c_prev = g0;
    for (uint32_t j = 0; j < n_r; ++j) {
        const uint32_t c_next = j + 1u < n_r ? cut_of(j + 1u) : 0xFFFFFFFFu;
        RangeRun r{};
        r.g_begin = (j == 0u || c_prev - g0 <= warm) ? g0 : c_prev - warm;
        r.g_stop = c_next;
        r.g_seg0 = g0;
        r.emit_from = c_prev;
        r.flags = j + 1u == n_r ? kRunLast : 0u;
        r.split = split;
        runs[run_base + j] = r;
        // (what range j - 1 holds when it stops at this range's cut against what this range holds when it reaches it)
        if (j) cuts[cut_base + j - 1u] = make_uint2(run_base + j - 1u, run_base + j);
        c_prev = c_next;
    }
}

// (option debug = 2: per tier the placed segment with the most probe positions and the one with the most hits that was NOT cut
// -- top[2 t] and top[2 t + 1] = figure << 32 | segment)
__global__ __launch_bounds__(256) void top_uncut_kernel(const unsigned long long *__restrict__ n_seg_ptr, const uint32_t *__restrict__ keys,
                                                       const uint2 *__restrict__ seg_info, unsigned long long *__restrict__ top) {
    const unsigned long long sj = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (sj >= *n_seg_ptr) return;
    const uint32_t tier = keys[sj] >> 29;
    if (tier >= (uint32_t)kTiers) return;
    const uint2 info = seg_info[sj];
    atomicMax(&top[2u * tier], (unsigned long long)(info.y & 0x7FFFFFFFu) << 32 | sj);
    atomicMax(&top[2u * tier + 1u], (unsigned long long)info.x << 32 | sj);
}

template <uint32_t W>  // (words per dumped arm: kDumpWords)
__global__ __launch_bounds__(256) void validate_cuts_kernel(const uint2 *__restrict__ cuts, const uint32_t *__restrict__ run_meta,
                                                           const uint32_t *__restrict__ run_dump, uint32_t *__restrict__ cut_ok) {
    constexpr uint32_t Q = W / 4u;  // 16-byte quarters of an arm
    constexpr uint32_t kSlots = 16384;  // > 3 x kRunDumpCap
    __shared__ uint32_t s_tab[kSlots];
    __shared__ uint32_t s_ok, s_oldest;
    const uint2 cut = cuts[blockIdx.x];
    // (x: the run in front of the cut, its end state; y: the run behind it, its state at the cut)
    const uint32_t *ma = run_meta + (size_t)cut.x * 16, *mb = run_meta + (size_t)cut.y * 16 + 8;
    const uint32_t n = ma[0];
    const bool meta_ok = n == mb[0] && n <= kRunDumpCap && ma[2] == mb[2] && ma[3] == mb[3] && !ma[4] && !run_meta[(size_t)cut.y * 16 + 4];
    for (uint32_t j = threadIdx.x; j < kSlots; j += blockDim.x) s_tab[j] = 0u;
    if (threadIdx.x == 0) {
        s_ok = meta_ok ? 1u : 0u;
        s_oldest = 0xFFFFFFFFu;
    }
    __syncthreads();
    {   // the oldest arm the range in front of the cut holds there (its creation number: where in the segment it was born): a
        // run that is to hold it at the cut must start in front of that probe -- what the host sizes the next warm-up by
        const uint4 *da = reinterpret_cast<const uint4 *>(run_dump + (size_t)cut.x * 2 * kRunDumpCap * W);
        uint32_t oldest = 0xFFFFFFFFu;
        for (uint32_t j = threadIdx.x; j < min(n, kRunDumpCap); j += blockDim.x) oldest = min(oldest, da[Q * j].x);
        if (oldest != 0xFFFFFFFFu) atomicMin(&s_oldest, oldest);
    }
    if (meta_ok) {
        const uint4 *da = reinterpret_cast<const uint4 *>(run_dump + (size_t)cut.x * 2 * kRunDumpCap * W);
        const uint4 *db = reinterpret_cast<const uint4 *>(run_dump + ((size_t)cut.y * 2 + 1) * kRunDumpCap * W);
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
            uint32_t h = (da[Q * j].x * 2654435761u) >> 18;
            while (atomicCAS(&s_tab[h], 0u, j + 1u) != 0u) h = (h + 1u) & (kSlots - 1u);
        }
        __syncthreads();
        bool ok = true;
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
            const uint4 b0 = db[Q * j];
            uint32_t h = (b0.x * 2654435761u) >> 18;
            bool found = false;
            for (uint32_t probe = 0; probe < kSlots; ++probe) {
                const uint32_t e = s_tab[h];
                if (!e) break;
                const uint4 a0 = da[Q * (e - 1u)];
                if (a0.x == b0.x) {  // (creation numbers are unique within a dump)
                    found = a0.y == b0.y && a0.z == b0.z && a0.w == b0.w;
                    for (uint32_t q = 1; q < Q; ++q) {
                        const uint4 a = da[Q * (e - 1u) + q], b = db[Q * j + q];
                        found = found && a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
                    }
                    break;
                }
                h = (h + 1u) & (kSlots - 1u);
            }
            ok = ok && found;
        }
        if (!ok) s_ok = 0u;
    }
    __syncthreads();
    // (bit 0: the cut holds; above it: needle offset, counted from the segment's first probe, at which the oldest arm was born --
    // all ones: no arm)
    if (threadIdx.x == 0) cut_ok[blockIdx.x] = s_ok | ((s_oldest >> 10) << 1);
}

// run_fix[run]: what is added to the family ordinals of the run's records; ~0u: the run's records are dropped; ~0u - 1: not
// decided yet (left as they are for a later pass)
__global__ __launch_bounds__(256) void fixup_records_kernel(SdRec *__restrict__ recs, unsigned long long n, const uint32_t *__restrict__ run_fix) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SdRec &r = recs[i];
    if (r.g_start == kVoidStart || r.pad == 0u) return;
    const uint32_t f = run_fix[r.pad - 1u];
    if (f == 0xFFFFFFFEu) return;
    if (f == 0xFFFFFFFFu) r.g_start = kVoidStart;
    else r.fam_seq += f;
    r.pad = 0u;
}

}  // namespace asgart
