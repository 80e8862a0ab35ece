// tiers.hpp -- the table of the extension tiers; tiers.hip has the host code that plans their streams.
#pragma once
#include "extend_common_dev.hpp"
#include "extend_heavy_dev.hpp"

namespace asgart {

// ---- the extension tiers ---------------------------------------------------------------------------------------------------
// What a tier is, stated once.  Placement (place), every launch (launch_kernel), the statistics (finish_tiers) and the
// estimates of the tier plan (plan_estimates) read this table and nothing else; which stream a tier runs on is tier_plan's
// business (tiers.hip).
enum class TierKernel {
    none,          // the tier stays empty
    wave,          // extend_kernel: one wave per segment, arms in registers / LDS arrays
    fast,          // extend_fast_kernel: arm-resident, one barrier per step
    k8,            // extend_k8_kernel: arm-resident, specialised waves (two of the sixteen hold no arms)
    heavy_lds,     // extend_heavy_kernel MODE 0: arms in LDS arrays (launch_shape takes MODE from the order of these three)
    heavy_hybrid,  // ... MODE 1: hot fields in LDS, (rs, le) in HBM scratch; 16-bit gap / pend
    heavy_hbm      // ... MODE 2: arms in HBM scratch, a slice of heavy_cap arms per workgroup
};
static_assert((int)TierKernel::heavy_hybrid == (int)TierKernel::heavy_lds + 1 && (int)TierKernel::heavy_hbm == (int)TierKernel::heavy_lds + 2,
              "extend_heavy_kernel's MODE is the distance from heavy_lds");
struct TierShape {
    TierKernel kernel;
    int threads;              // per workgroup
    int layers, slots;        // arm layers (arms per thread) x arm-holding slots per layer: the arms it holds
    int hits, rows;           // hits staged per probe; table rows (arm-resident kernels)
    int wg_per_cu;            // workgroups of this shape a compute unit holds (LDS / registers)
    int grid;                 // default grid
    int64_t Options::*widen;  // the option that lets it accept segments whose arm BOUND is that percentage of cap() (null: none)
    bool early;               // what it gives up on is re-run as soon as it has ended (run_tiers)
    double profile_ms;        // its duration before a call has measurements (plan_estimates)
    uint32_t tail_hits = 0;   // > 0: the tail rule's threshold (place_tier): segments with this many hits and more leave the tier
    double tail_profile_ms = 0.0;  // ... and its duration without them: what replaces profile_ms in a call where the rule is in force
    constexpr uint32_t cap() const { return (uint32_t)(layers * slots); }
};
// shape[t][0]: tier t of the arm-resident set, shape[t][1]: of the LDS-array set, which takes over with
// max_cardinality > 1024, option arms_kernel = 0 (tests) or a text of 2^42 bases (the arm-resident kernels pack a
// position into 42 bits of a table entry).  shape[0]: the runs over ranges of the cut segments.
template <class SlotT>
struct TierTable {
    static constexpr bool k32 = sizeof(SlotT) == 4;  // 64-bit positions: fewer arms per thread, smaller tables
    static constexpr int kLong = k32 ? 2048 : 1024;  // table rows of the long shapes
    // (an empty entry is never placed into and never launched: launch_kernel refuses)
    static constexpr TierShape kNone = {TierKernel::none, 0, 0, 0, 0, 0, 1, 0, nullptr, false, 0.0};
    static constexpr TierShape kWave = {TierKernel::wave, 64, 1, 256, kHitBatch, 0, 11, 256 * 8, nullptr, false, 3.4};
    static constexpr TierShape kHbm = {TierKernel::heavy_hbm, kHeavyThreads, 1, 1, kHitBatch, 0, 1, 256, nullptr, false, 56.6};
    static constexpr TierShape kK8 = {TierKernel::k8, 1024, k32 ? 5 : 4, 896, kHitBatch, kLong, 1, 256, &Options::cap3_pct, true, 56.6};
    // profile_ms: the GRCh38-shaped profile (profiles/tail_up_ab.json; the rows of tiers 2 and 5 and of the runs as
    // profiles/r06_cfg4_tier_cu_seconds.json had them, which the new measurements bear out): the longest segments of tiers
    // 2, 4 and 5, tier 1's work over its compute units, the runs' duration; tiers 3 and 6 (tier 7 as tier 6) the longer of
    // their longest segment and the step's 14.5 CU-seconds spread over the chip (remember_plan_estimates).
    // tail_hits of tier 4 (place_tier; 32-bit positions only: nothing of that size with 64-bit positions is measured).  What
    // stays in tier 4 runs behind another tier, which ends 56-60 ms after the launches, and should end with the runs at 67 ms:
    // about 7 ms, well inside the quarter of the runs that bounds a thresholded tier.  Tier 4's segments on its own kernel,
    // ms / hits by rank: 35.5 / 471 K, 21.1 / 223 K, 13.1 / 145 K, 9.0 / 97 K, 7.05 / 35 K -> 36 000 hits.  Measured: 58 of
    // 9 543 segments move, what stays takes 8.7 ms (tail_profile_ms: tier 4's estimate in a call where its threshold is in
    // force; profile_ms where it is not).  Tiers 2 and 5 keep their segments (DESIGN_HISTORY.md has the whole derivation).
    // {kernel, threads, layers, slots, hits, rows, wg_per_cu, grid, widen, early, profile_ms[, tail_hits, tail_profile_ms]}
    static constexpr TierShape shape[kTiers + 1][2] = {
        // the runs over ranges: tier 3's kernel, one workgroup per run (no default grid)
        {{kK8.kernel, kK8.threads, kK8.layers, kK8.slots, kK8.hits, kK8.rows, 1, 0, nullptr, false, 67.0}, kNone},
        // 1: the common case; placement never puts a segment busier than kTier1MaxSum on a single wave
        {kWave, kWave},
        // 2: one wave, probes with up to 512 hits | the block-cooperative kernel, 256 threads per segment
        {{TierKernel::fast, 64, k32 ? 8 : 5, 64, 512, 256, 8, 256 * 8, nullptr, false, 51.8},
         {TierKernel::heavy_lds, kMidThreads, 1, 768, kHitBatch, 0, 3, 256 * 3, nullptr, false, 51.8}},
        // 3: the LONG DENSE segments.  It accepts what tier 6 would accept by the bound (a long segment is no less safe
        // there), but never more than cap3_pct of its own capacity: with 64-bit positions it holds fewer arms than tier 6,
        // and what it gives up on is re-run from the start.  (The bound of a tandem array is three to four times what it
        // really holds.)
        // (A half shape -- 512 threads, 5 x 384 slots, 75 KB of LDS, two workgroups per compute unit -- was measured in
        // round 6: 37 % less compute-unit time per hit-probe, 25 % more wall time, and the 208 segments of a GRCh38-sized
        // step whose arms do not fit it fall to tier 6's kernel, one of them for 145 ms: the step doubled.
        // DESIGN_HISTORY.md.)
        {kK8, kNone},
        // 4: cold fields in LDS, probes with up to 512 hits | 32-bit positions: 3072 * 40 B + hits + scratch = 128 KiB of
        // LDS, 64-bit: 2048 * 60 B + hits + scratch = 132 KiB
        {{TierKernel::fast, 256, k32 ? 4 : 2, 256, 512, 512, 4, 256 * 4, &Options::cap45_pct, false, 35.5, k32 ? 36000u : 0u, 8.7},
         {TierKernel::heavy_lds, kHeavyThreads, 1, k32 ? 2432 : 1664, kHitBatch, 0, 1, 256, nullptr, false, 35.5}},
        // 5
        {{TierKernel::fast, 512, k32 ? 4 : 2, 512, kHitBatch, 1024, 2, 256 * 2, &Options::cap45_pct, false, 53.0}, kNone},
        // 6: the long sparse segments.  The window bound is pessimistic for tandem arrays (hits extend arms there) and the
        // HBM tier is several times slower per probe: tier 6 also takes segments whose bound exceeds its capacity, by up
        // to 40 % (a real overflow falls through the cascade).  With 64-bit positions the HBM tier is an order of
        // magnitude slower per probe and the bound three to four times what a segment really holds -- at cfg5 every
        // segment that went to tier 7 by its bound peaked below 4 096 arms: cap6w_pct.  | by 7/5, in place()
        {{TierKernel::fast, 1024, k32 ? 5 : 4, 1024, kHitBatch, kLong, 1, 256, k32 ? &Options::cap6_pct : &Options::cap6w_pct, true, 56.6},
         {TierKernel::heavy_hybrid, kHeavyThreads, 1, k32 ? 4608 : 3072, kHitBatch, 0, 1, 256, nullptr, true, 56.6}},
        // 7: whatever is left (place() sizes its slices and its grid, at most this one, by the bound on the live arms of
        // ANY segment)
        {kHbm, kHbm},
    };
    static constexpr int kRunsTier = 3;  // the tier whose kernel the runs run and whose statistics they are counted with
};
template <class SlotT>
constexpr bool tier_caps(int set, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t c4, uint32_t c5, uint32_t c6) {
    const uint32_t want[kTiers] = {0, c1, c2, c3, c4, c5, c6};
    for (int t = 1; t < kTiers; ++t)
        if (TierTable<SlotT>::shape[t][set].cap() != want[t]) return false;
    return true;
}
static_assert(tier_caps<uint32_t>(0, 256, 512, 4480, 1024, 2048, 5120) && tier_caps<uint64_t>(0, 256, 320, 3584, 512, 1024, 4096),
              "capacities of the arm-resident set");
static_assert(tier_caps<uint32_t>(1, 256, 768, 0, 2432, 0, 4608) && tier_caps<uint64_t>(1, 256, 768, 0, 1664, 0, 3072),
              "capacities of the LDS-array set");
constexpr uint32_t kTier1MaxSum = 20000;  // placement: busier segments never run on a single wave

// The extension tiers' streams of one call (host code, tiers.hip; asgart_tier_plan): stream_of[t - 1] = 0 for the main
// stream, s for tier stream s (1 .. min(6, budget)), -1 for a tier without work; launch[] = the tiers with work in launch
// order (which is also the order within each stream: longest estimate first), 0 behind them.
int32_t tier_plan(int budget, const uint64_t *n_work, int64_t tier_order, const double *est_ms, double main_ms,
                  int32_t *stream_of, int32_t *launch);

}  // namespace asgart
