// search_call.hpp -- the state of one search call and the list of its stages; each stage is defined in a header of its
// own (call_setup.hpp, call_front.hpp, call_place.hpp, call_tiers.hpp, call_join.hpp, call_records.hpp), run() in
// pipeline.hip.
#pragma once
#include "pipeline_dev.hpp"
#include "extend_wave_dev.hpp"
#include "extend_heavy_dev.hpp"
#include "extend_fast_dev.hpp"
#include "extend_k8_dev.hpp"
#include "tiers.hpp"
#include "watchdog.hpp"
#include "call_profile.hpp"

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <thread>
#include <utility>

namespace asgart {

// One job over the probes of n_passes passes (orientations) of the same chunk list: sts[p] differ in reverse /
// complement only (the caller has checked); fams[p] receives pass p's families (null: none wanted -- the CSR surface).
// The stages of a call, in the order run() takes them:
//   setup          chunk table, probe numbering, this shard's own range
//   set_window     the windows of this attempt (halos grow on retry), RunParams
//   front          probe search, row offsets + segment starts, hit rows            (the HBM-bound, chip-wide part)
//   csr_out        asgart_probe_hits only: the per-probe hit rows to the host
//   place          per segment: arm bound -> tier, barren tests, long segments cut into ranges, lists sorted by cost
//   run_tiers      every extension tier and the runs over ranges launched together; early re-runs of tiers 3 and 6
//   join_ranges    cuts checked, family ordinals of the ranges chained, refused segments run again
//   finish_tiers   statistics, the cascade of what overflowed
//   records        records -> reference order -> families per pass on the host
//   fill_stats
template <class SlotT>
struct SearchCall {
    int32_t setup();                  // call_setup.hpp
    void set_window();
    int32_t front(bool *ambiguous);   // call_front.hpp
    int32_t csr_out();
    int32_t place();                  // call_place.hpp
    int32_t run_tiers(int attempt);   // call_tiers.hpp
    int32_t join_ranges();            // call_join.hpp
    int32_t finish_tiers();           // call_tiers.hpp
    int32_t records();                // call_records.hpp
    int32_t fill_stats();
    int32_t run();                    // pipeline.hip

    // ---- the call ---------------------------------------------------------------------------------------------------------
    asgart_index *const idx;
    SearchCtx &cx;
    const uint64_t *const chunks;
    const int64_t n_chunks_pass;
    const asgart_settings *const sts;
    const int32_t n_passes, shard, n_shards;
    const bool want_csr;
    asgart_families *const *const fams;
    std::vector<uint8_t> *const status_out;
    std::vector<uint64_t> *const rowoff_out, *const hits_out;
    Workspace &w;
    const hipStream_t s;
    const asgart_settings *const st;
    const bool fam_out;
    const int64_t n_chunks;      // entries of the chunk table: the chunk list once per pass
    const uint64_t k, step, n;
    const Options opt;           // options cannot change while this call holds a context
    const TailUp tail_up;        // (nor the tail rule's settings)
    static constexpr size_t kCtrBytes = (size_t)CT_COUNT * 8;
    static constexpr size_t kSplitMirror = 512 << 10;  // (option split: host copy of Workspace::split_buf)
    using Tiers = TierTable<SlotT>;
    static constexpr int caph = (int)Tiers::shape[6][1].cap();  // (its HBM scratch is reserved whichever set runs)
    // ---- set up once (setup) --------------------------------------------------------------------------------------------
    bool nothing_to_do = true;
    size_t ch_bytes = 0;
    unsigned long long *h_ctr = nullptr, *h_scalar = nullptr;  // pinned: the counters read back; source of small host-to-device updates
    uint64_t *h_start = nullptr, *h_len = nullptr;
    uint32_t *h_pbase = nullptr;
    char *h_split = nullptr;
    std::vector<uint32_t> lp;    // probes of the chunk list, counted from the start of a pass
    uint32_t Ppass = 0, P = 0, own_lo = 0, own_hi = 0, lo_lim = 0, hi_lim = 0, K = 0;
    uint64_t look_back = 0, look_ahead = 0, call_sig = 0;
    uint64_t *d_start = nullptr, *d_len = nullptr;
    uint32_t *d_pbase = nullptr;
    std::chrono::steady_clock::time_point t_host0, t_launch;
    // ---- per window (set_window, front) ---------------------------------------------------------------------------------
    RunParams rp;
    uint32_t W = 0, W_probes = 0;
    unsigned long long *d_ctr = nullptr;
    IndexView<SlotT> ix;
    SlotT *p_lo = nullptr, *hits = nullptr;
    uint32_t *p_raw = nullptr, *p_filt = nullptr, *seg_list = nullptr;
    unsigned long long *row_off = nullptr;
    uint64_t total_hits = 0, n_seg = 0, n_overflow = 0, n_heavy = 0;
    bool progress_given = false;
    // ---- placement (place) ----------------------------------------------------------------------------------------------
    uint64_t rec_cap = 0;
    const SdRec *h_recs = nullptr;  // sorted records on the host (pinned staging of the context)
    size_t n_hrec = 0;
    bool arms_kernel = false, split_on = false;
    uint32_t tier_cap[kTiers + 1] = {};
    uint32_t tail_hits[kTiers + 1] = {};  // the tail rule's thresholds of THIS call (0: tier t keeps its segments), place()
    char *d_split = nullptr;
    const uint32_t *order = nullptr;
    uint64_t n_t[kTiers] = {}, seg_off[kTiers + 1] = {};
    uint64_t h_tp[kTiers] = {}, h_th[kTiers] = {};  // (option debug: hit-probes and hits per tier, as placed)
    const unsigned long long *h_split_hdr = nullptr;
    uint32_t n_runs = 0, n_cuts = 0, n_splits = 0;
    std::vector<SplitSeg> split_segs;
    uint32_t *ovf[kTiers] = {};  // ovf[t-1]: segments tier t gave up on
    uint64_t heavy_cap64 = 0;
    unsigned n_wg7 = 1;
    size_t region = 0;
    char *scratch6 = nullptr, *scratch7 = nullptr;
    // ---- the tiers (run_tiers .. finish_tiers) ---------------------------------------------------------------------------
    ExtParams<SlotT> base{};  // what every launch of this attempt shares (run_tiers); launch_kernel adds the work list
    hipStream_t tier_stream[kTiers + 1] = {};
    bool tier_ran[kTiers + 1] = {};  // launched by run_tiers (its event in cx.tier_ev is this call's)
    uint64_t early_n[kTiers + 1] = {};
    double ms_tier2 = 0.0, ms_longest_tier = 0.0, ms_longest_segment = 0.0;
    uint64_t n_split_segments = 0, n_split_refused = 0;

    SearchCall(asgart_index *idx_, SearchCtx &cx_, const uint64_t *chunks_, int64_t n_chunks_pass_, const asgart_settings *sts_,
               int32_t n_passes_, int32_t shard_, int32_t n_shards_, bool want_csr_, asgart_families *const *fams_,
               std::vector<uint8_t> *status_out_, std::vector<uint64_t> *rowoff_out_, std::vector<uint64_t> *hits_out_)
        : idx(idx_), cx(cx_), chunks(chunks_), n_chunks_pass(n_chunks_pass_), sts(sts_), n_passes(n_passes_), shard(shard_),
          n_shards(n_shards_), want_csr(want_csr_), fams(fams_), status_out(status_out_), rowoff_out(rowoff_out_),
          hits_out(hits_out_), w(cx_.ws), s(cx_.stream), st(&sts_[0]), fam_out(fams_ != nullptr),
          n_chunks(n_chunks_pass_ * (int64_t)n_passes_), k(sts_[0].probe_size), step(sts_[0].probe_size / 2),
          n((uint64_t)idx_->n), opt(idx_->opt), tail_up(idx_->tail_up) {}

    uint32_t pass_of_probe(uint32_t g) const { return std::min<uint32_t>(g / K, (uint32_t)n_passes - 1u); }
    uint32_t pass_offset(uint32_t g) const { return lo_lim + (g - pass_of_probe(g) * K); }  // from the start of its pass
    const TierShape &shape(int t) const { return Tiers::shape[t][arms_kernel ? 0 : 1]; }  // (t = 0: the runs over ranges)
    bool tier_enabled(int t) const { return t >= 1 && t <= kTiers && tier_cap[t] != 0; }
    // where what tier src gave up on is run again: the next tier that is in use and holds more arms
    int next_holding_more(int src) const { return asgart::next_holding_more(tier_cap + 1, src); }
    double since_launch() const {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_launch).count();
    }
    void signal_progress() {  // (only single-pass calls have a progress array)
        fill_progress(cx.progress, h_len, 1, n_chunks_pass, *st);
        progress_given = true;
    }

    // Workspace::split_buf: [4 counters (u64): runs, cuts, split segments, work cursor | runs | cuts | split segments |
    // run states | verdicts per cut | per run: what is added to its records' family ordinals | segments to run again | range
    // size chosen | what earlier calls found out about segments with a cut that did not hold]
    static constexpr uint32_t kMaxRuns = 4096, kMaxCuts = 2048, kMaxSplits = 1024;
    static constexpr size_t kOffRuns = 64, kOffCuts = kOffRuns + kMaxRuns * sizeof(RangeRun), kOffSplits = kOffCuts + kMaxCuts * 8,
                     kOffMeta = kOffSplits + kMaxSplits * sizeof(SplitSeg), kOffOk = kOffMeta + kMaxRuns * 64,
                     kOffFix = kOffOk + kMaxCuts * 4, kOffAgain = kOffFix + kMaxRuns * 4, kOffChoice = kOffAgain + kMaxSplits * 4,
                     kOffBlocked = kOffChoice + 128, kSplitBytes = kOffBlocked + kSplitBlockedMax * sizeof(BlockedSeg);
    static_assert(sizeof(SplitChoice) <= 128 && kOffChoice % 8 == 0, "split choice");
    static_assert(kSplitBytes <= kSplitMirror, "split mirror");

    // What one launch works through.  Every launch site builds its own: nothing is inherited from an earlier launch.
    struct WorkList {
        const uint32_t *list;             // the segments (the runs over ranges: null, the runs are the list)
        const unsigned long long *count;  // device count of the entries
        unsigned long long *cursor;       // work-fetch cursor
        int ovf_into;                     // what the launch gives up on goes where tier ovf_into's own goes
        uint32_t cap_limit;               // test_cap(), or 0xFFFFFFFF for a re-run of what overflowed
        char *scratch = nullptr;          // HBM region of the LDS-array kernels (null: the tier's own)
    };
    // option test_cap_limit (tests): shrink the tiers' capacity to exercise the cascade
    uint32_t test_cap() const { return opt.test_cap_limit >= 0 ? (uint32_t)opt.test_cap_limit : 0xFFFFFFFFu; }

    // tier t's busy time or workgroups (ct1: CT_BUSY1, CT_WGS1) and its longest segment, the runs over ranges counted with
    // the long-segment tier whose kernel they run
    unsigned long long tier_sum(int ct1, int t) const { return h_ctr[ct1 + t - 1] + (t == Tiers::kRunsTier ? h_ctr[ct1 + kRunsStat - 1] : 0ull); }
    unsigned long long tier_longest(int t) const { return std::max(h_ctr[CT_SEGMAX1 + t - 1], t == Tiers::kRunsTier ? h_ctr[CT_SEGMAX1 + kRunsStat - 1] : 0ull); }
    // The statistics and the plan's estimates count every tier with the ARM-RESIDENT set's workgroups per compute unit,
    // compute units and profile, whichever set runs: so they always have, and with the LDS-array set's own figures
    // (3, 1, 1 for tiers 2, 4, 6) tier_plan would pack the streams of such a call differently.
    static const TierShape &stat_shape(int t) { return Tiers::shape[t][0]; }

    // ---- the launches (call_tiers.hpp; apply_fix: call_join.hpp) ----------------------------------------------------------
    template <int T, int SET>
    static void launch_shape(const ExtParams<SlotT> &p, unsigned grid, hipStream_t st);
    template <int... I>
    static void launch_entry(int entry, std::integer_sequence<int, I...>, const ExtParams<SlotT> &p, unsigned grid, hipStream_t st);
    int32_t launch_kernel(int tier, const WorkList &wl, uint64_t n_items, hipStream_t st);
    int32_t launch_runs(uint32_t n_items);
    int32_t launch_tier(int tier);
    int32_t rerun_list(int tier, const uint32_t *list, uint64_t n, int ovf_into, uint32_t cap_limit);
    int32_t apply_fix();
    uint64_t plan_sig() const;
    void plan_estimates(double *est) const;
    void remember_plan_estimates();
};

}  // namespace asgart
