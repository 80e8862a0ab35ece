// tiers.hip -- the host code of the extension tiers: which stream each tier of a call runs on (tier_plan), and what the
// tier table (tiers.hpp) says before a call has measurements.  Host only: nothing is launched from here.
#include "tiers.hpp"

#include <algorithm>

namespace asgart {

// The tiers' streams of a call.  Streams of one priority share the process's queues, and
// kernels of streams on one queue run one after the other -- a tier behind another waits for that tier's longest
// segment.  So a call gets at most one tier stream per queue (min(6, budget)) and tiers that must share one are put
// behind each other knowingly: longest-processing-time packing of the tiers' estimated durations (each the longer of
// its longest segment and its work spread over the compute units it can hold) onto the tier streams, and -- when the
// process has two queues or more -- onto the main stream behind the runs over ranges.  Longest first (ties: the launch
// order), each onto the least-loaded stream (ties: tier streams in order, then the main stream), and behind what that
// stream already holds.  Every tier with work runs exactly once, the tiers option tier_order names and then the rest.
// With one queue the plan is that single chain (the main stream stays free for the other call context).
// Bound: the most loaded stream carries at most main_ms + total / (number of streams) + the largest single estimate.
int32_t tier_plan(int budget, const uint64_t *n_work, int64_t tier_order, const double *est_ms, double main_ms,
                  int32_t *stream_of, int32_t *launch) {
    constexpr int kT = 7;
    if (budget < 1 || !n_work || !est_ms || !stream_of || !launch || !(main_ms >= 0.0) || tier_order < 1 ||
        tier_order > 7777777) {
        set_error("asgart_tier_plan: bad argument");
        return ASGART_E_ARG;
    }
    for (int t = 0; t < kT; ++t)
        if (!(est_ms[t] >= 0.0) || est_ms[t] > 1e12) {
            set_error("asgart_tier_plan: estimate of tier %d is not a finite duration", t + 1);
            return ASGART_E_ARG;
        }
    int digits[kT] = {}, n_digits = 0;
    for (int64_t v = tier_order; v; v /= 10) {
        if (v % 10 < 1 || v % 10 > kT || n_digits == kT) {
            set_error("asgart_tier_plan: tier_order digits must be tiers 1..7");
            return ASGART_E_ARG;
        }
        digits[n_digits++] = (int)(v % 10);
    }
    int order[kT], n = 0;
    bool seen[kT + 1] = {};
    for (int i = n_digits - 1; i >= 0; --i)
        if (!seen[digits[i]]) {
            seen[digits[i]] = true;
            if (n_work[digits[i] - 1]) order[n++] = digits[i];
        }
    for (int t = 1; t <= kT; ++t)
        if (!seen[t] && n_work[t - 1]) order[n++] = t;
    for (int i = 0; i < kT; ++i) stream_of[i] = -1;
    int by_cost[kT], depth[kT + 1] = {}, slot[kT + 1] = {};
    std::copy(order, order + n, by_cost);
    std::stable_sort(by_cost, by_cost + n, [&](int a, int b) { return est_ms[a - 1] > est_ms[b - 1]; });
    const int n_st = std::min(budget, SearchCtx::kMaxTierStreams);
    const bool main_ok = budget >= 2;
    double load[SearchCtx::kMaxTierStreams + 1] = {main_ms};
    int on[SearchCtx::kMaxTierStreams + 1] = {};
    for (int i = 0; i < n; ++i) {
        int best = 1;
        for (int q = 2; q <= n_st; ++q)
            if (load[q] < load[best]) best = q;
        if (main_ok && load[0] < load[best]) best = 0;
        const int t = by_cost[i];
        stream_of[t - 1] = best;
        depth[t] = on[best]++;
        load[best] += est_ms[t - 1];
    }
    // Launch: the first tier of every stream in the option's order, then the second ones, ...  Within a stream the
    // longer estimate goes first, so that its longest segment starts at once (a tier behind another on one queue starts
    // when that one has ended, and the tiers that hold whole compute units end late when they share the chip).  With
    // one queue the chain is serial whatever its order, and it keeps the option's.
    for (int i = 0; i < n; ++i) slot[order[i]] = budget == 1 ? i : depth[order[i]] * kT + i;
    std::sort(order, order + n, [&](int a, int b) { return slot[a] < slot[b]; });
    for (int i = 0; i < kT; ++i) launch[i] = i < n ? order[i] : 0;
    return 0;
}

}  // namespace asgart

using namespace asgart;

extern "C" {

int32_t asgart_tier_plan(int32_t budget, const uint64_t *n_work, int64_t tier_order, const double *est_ms, double main_ms,
                         int32_t *stream_of, int32_t *launch) {
    return asgart::tier_plan(budget, n_work, tier_order, est_ms, main_ms, stream_of, launch);
}

int32_t asgart_tier_profile(double *profile_ms, uint64_t *tail_hits) {
    if (!profile_ms || !tail_hits) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    for (int t = 0; t <= kTiers; ++t) {
        const TierShape &sh = TierTable<uint32_t>::shape[t][0];
        profile_ms[t] = sh.tail_hits && sh.tail_profile_ms > 0.0 ? sh.tail_profile_ms : sh.profile_ms;
        tail_hits[t] = TierTable<uint32_t>::shape[t][0].tail_hits;
    }
    return 0;
}

}  // extern "C"
