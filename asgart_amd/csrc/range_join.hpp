// range_join.hpp -- the host rules of the long segments run as ranges (option split), as plain functions: which ranges of
// a cut segment stand when a cut did not hold (join_segment, settle_tail), which warm-up the index remembers for the
// segment (split_warm_next), and the index's memory of such segments (remember_split, blocked_in_call).  No HIP in here:
// join_ranges (call_join.hpp) and place (call_place.hpp) call these between their launches, asgart_join_cuts and
// asgart_split_warm_next (search_abi.hip) expose them to host tests.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace asgart {

// ---- one cut segment: what stands ---------------------------------------------------------------------------------------
// The per-run entry of the fix table (fixup_records_kernel): what is added to the family ordinals of the run's records,
// or one of these two.
constexpr uint32_t kFixHeld = 0xFFFFFFFEu;     // the records wait: decided when the segment's tail run has come back
constexpr uint32_t kFixDropped = 0xFFFFFFFFu;  // the records are dropped
enum class JoinAction : int32_t {
    joined = 0,      // every cut held: the ranges' records stand
    tail_run = 1,    // ranges 0 .. f stand, ONE more run covers the rest of the segment
    whole_again = 2  // nothing stands: the whole segment runs again on the ordinary kernel
};
struct JoinVerdict {
    uint32_t f;          // the first cut that did not hold (the number of cuts: every cut held)
    JoinAction action;
    uint32_t tail_base;  // tail_run: the family-ordinal base of the tail run, the flushes of ranges 0 .. f
};
// A segment of R ranges.  cut_held[j] bit 0: cut j, between ranges j and j + 1, held (R - 1 verdicts of
// validate_cuts_kernel); flush[j * flush_stride]: the families range j flushed; last_gave_up: the run over the last range
// gave up (more arms than the long shape holds: the cascade's business).
// Every cut of a segment held: the family ordinals of range j count on from the flushes of ranges 0 .. j - 1.
// The first cut that did not hold is cut f: ranges 0 .. f stand (range f started from a state that was checked),
// the records of the ranges behind it are dropped, and ONE more run covers the rest -- from where range f started
// (it passes cut f in the checked state, so it is exact from there on), reporting from cut f + 1 to the segment's
// end.  f = 0, or a run that gave up: the segment runs again as a whole on the ordinary kernel.
// fix[R]: the ranges' entries of the fix table; held[R]: with tail_run, the bases ranges 0 .. f get when the tail run
// has come back (settle_tail).
inline JoinVerdict join_segment(uint32_t R, const uint32_t *cut_held, const uint32_t *flush, size_t flush_stride, bool last_gave_up,
                                uint32_t *fix, uint32_t *held) {
    const uint32_t n_cuts = R - 1;
    uint32_t f = n_cuts;
    for (uint32_t j = 0; j < n_cuts; ++j)
        if (!(cut_held[j] & 1u)) {
            f = j;
            break;
        }
    const bool ok = f == n_cuts && !last_gave_up;
    if (f == n_cuts && last_gave_up) f = 0;
    const bool tail = !ok && f > 0;
    JoinVerdict v{f, ok ? JoinAction::joined : tail ? JoinAction::tail_run : JoinAction::whole_again, 0u};
    uint32_t base = 0;
    for (uint32_t j = 0; j < R; ++j) {
        // (ranges in front of a cut that did not hold: decided when the run over the rest has come back)
        fix[j] = ok ? base : (tail && j <= f) ? kFixHeld : kFixDropped;
        if (tail && j <= f) held[j] = base;
        base += flush[(size_t)j * flush_stride];
        if (tail && j == f) v.tail_base = base;
    }
    return v;
}
// The tail run of a segment has come back: ranges 0 .. f get their bases (fix[f + 1], from join_segment's held) and the
// tail run its own (*tail_fix).  A tail run that gave up -- more arms than the long shape holds --: everything the
// segment's runs wrote is dropped and the whole segment goes the cascade's way.
inline JoinAction settle_tail(uint32_t f, const uint32_t *held, uint32_t tail_base, bool tail_gave_up, uint32_t *fix, uint32_t *tail_fix) {
    *tail_fix = tail_gave_up ? kFixDropped : tail_base;
    for (uint32_t j = 0; j <= f; ++j) fix[j] = tail_gave_up ? kFixDropped : held[j];
    return tail_gave_up ? JoinAction::whole_again : JoinAction::tail_run;
}

// ---- what the index remembers about a segment a cut of which did not hold ---------------------------------------------------
// allowed: how many of its cuts, from the start, held; warm_used: the warm-up its ranges had (0: the warm-up is not the
// matter); need: how far in front of the failed cut the oldest arm of the range before it was born (probes; 0: it held no
// arm) -- a run that is to hold that arm at the cut has to start in front of its birth.  While a warm-up of that size is
// still worth a range (no longer than two ranges, nor than option split_warm_max) the next call gives this segment's
// ranges that much and plans all its cuts again: a shard of a genome-sized call gets short ranges with short warm-ups,
// and with "only the cuts that held" the rest of such a segment became one long last range, the longest work item of the
// shard (81 ms of a 90-ms shard).  A cut that failed although every arm was born inside the warm-up (thresholds that had
// not settled) gets the longest warm-up that limit allows.  Beyond the limit -- the arms of a flat tandem array live from
// its first probe to its last, those of a chromosome run against its homologue for megabases: every run would walk the
// stretch again from its start -- only the cuts that held are planned again.
// The warm-up the segment's ranges get in the next call; 0: the call's own, and only the cuts that held.
inline uint32_t split_warm_next(uint32_t warm_used, uint32_t need, uint32_t range_len, uint64_t split_warm_max) {
    const uint64_t limit = std::min<uint64_t>(split_warm_max, 2ull * range_len);
    // (born inside the warm-up and still not the same arms: the longest warm-up a range is worth, at once -- a
    // doubling per call took a two-genome call, 2-3 s each, five calls to settle)
    const uint64_t want = need > warm_used ? (((uint64_t)need + 64u + 255u) & ~255ull) : (warm_used < limit ? limit : ~0ull);
    return (warm_used && want <= limit) ? (uint32_t)want : 0u;
}

// asgart_index::split_blocked holds these: orientation << 32 | first probe counted from the start of its pass, under
// which settings and chunk list (sig), how many of the segment's cuts, from the start, held (only those are planned
// again) and at which range length.  Cleared with the keys; the oldest entries age out.
struct SplitVerdict {
    uint64_t key, sig;
    uint32_t allowed, range_len;  // (the count belongs to the range length it was found at: one entry per segment and length)
    uint32_t warm;                // the warm-up this segment's ranges get from now on (0: the call's own)
};
constexpr uint32_t kPlanAllCuts = 0xFFFFFFFFu;  // SplitVerdict::allowed: every cut (kAllCuts of ranges_dev.hpp; call_join.hpp checks)
constexpr size_t kSplitVerdictsMax = 4096;
// A verdict about segment `key` of the calls with signature sig, found with ranges of range_len probes (the caller holds
// the index's lock).  warm_next from split_warm_next: with a warm-up all cuts are planned again.
inline void remember_split(std::vector<SplitVerdict> &list, uint64_t key, uint64_t sig, uint32_t range_len, uint32_t allowed,
                           uint32_t warm_next) {
    if (warm_next) allowed = kPlanAllCuts;
    // (one verdict per segment AND range length: calls of different shapes -- the passes as one job, a pass alone --
    // get different range lengths from the budget, and each shape keeps what it has learned)
    for (auto &b : list)
        if (b.key == key && b.sig == sig && b.range_len == range_len) {
            b.allowed = warm_next ? allowed : std::min(b.allowed, allowed);
            if (warm_next) b.warm = warm_next;
            return;
        }
    // (verdicts age out, oldest first: a forgotten one costs its segment one more refused cut, no more)
    if (list.size() >= kSplitVerdictsMax) list.erase(list.begin());
    list.push_back({key, sig, allowed, range_len, warm_next});
}
// The other side, place(): the verdicts that belong to a call -- its signature, the orientation of one of its passes
// (modes: 8 bits per pass), a first probe inside the stretch [lo_lim, hi_lim) of a pass that its windows hold -- the newest
// first, at most max_out of them: emit(pass, verdict).  Returns how many.
template <class Emit>
inline uint32_t blocked_in_call(const std::vector<SplitVerdict> &list, uint64_t sig, uint32_t modes, int32_t n_passes, uint32_t lo_lim,
                                uint32_t hi_lim, uint32_t max_out, Emit emit) {
    uint32_t n = 0;
    for (auto b = list.rbegin(); b != list.rend(); ++b)
        for (int32_t p = 0; p < n_passes && n < max_out; ++p)
            if (b->sig == sig && ((modes >> (8 * p)) & 0xFFu) == (uint32_t)(b->key >> 32) && (uint32_t)b->key >= lo_lim &&
                (uint32_t)b->key < hi_lim) {
                emit(p, *b);
                ++n;
            }
    return n;
}

}  // namespace asgart
