// call_tiers.hpp -- stages run_tiers and finish_tiers of a search call: every launch of an extension kernel, the
// cascade of what overflowed, and the estimates the tier plan starts from.
// Part of pipeline.hip, the one translation unit that launches the search kernels (search_call.hpp has the stage list).
#pragma once
#include "search_call.hpp"

namespace asgart {

// the kernel of one table entry: its template arguments are the entry's
template <class SlotT>
template <int T, int SET>
void SearchCall<SlotT>::launch_shape(const ExtParams<SlotT> &p, unsigned grid, hipStream_t st) {
    constexpr TierShape sh = Tiers::shape[T][SET];
    constexpr int cap = (int)sh.cap();
    if constexpr (sh.kernel == TierKernel::wave)
        extend_kernel<SlotT, cap><<<grid, sh.threads, 0, st>>>(p);
    else if constexpr (sh.kernel == TierKernel::fast)
        extend_fast_kernel<SlotT, sh.layers, sh.threads, sh.hits, sh.rows, 2><<<grid, sh.threads, 0, st>>>(p);
    else if constexpr (sh.kernel == TierKernel::k8)
        extend_k8_kernel<SlotT, sh.layers, sh.threads, sh.hits, sh.rows, 2, T == 0><<<grid, sh.threads, 0, st>>>(p);
    else if constexpr (sh.kernel != TierKernel::none)
        extend_heavy_kernel<SlotT, cap, sh.threads, (int)sh.kernel - (int)TierKernel::heavy_lds><<<grid, sh.threads, 0, st>>>(p);
}
template <class SlotT>
template <int... I>
void SearchCall<SlotT>::launch_entry(int entry, std::integer_sequence<int, I...>, const ExtParams<SlotT> &p, unsigned grid, hipStream_t st) {
    ((entry == I ? launch_shape<I / 2, I % 2>(p, grid, st) : void()), ...);
}

// one launch of tier `tier`'s kernel (0: the runs over ranges) over the first n_items of wl
template <class SlotT>
int32_t SearchCall<SlotT>::launch_kernel(int tier, const WorkList &wl, uint64_t n_items, hipStream_t st) {
    const bool runs = tier == 0;
    if (shape(tier).kernel == TierKernel::none) {  // (cannot happen: place() gives such a tier no segments and cuts no ranges)
        set_error("internal: tier %d has no kernel in this set, its %llu work items would be lost", tier, (unsigned long long)n_items);
        return ASGART_E_CAP;
    }
    // (statistics, segment clocks, heartbeats: the runs have a slot of their own and block 0, no tier's; the debug
    // output counts them with tier 3)
    const uint32_t stat = runs ? (uint32_t)kRunsStat : (uint32_t)tier;
    ExtParams<SlotT> p = base;
    p.runs = runs ? reinterpret_cast<const RangeRun *>(d_split + kOffRuns) : nullptr;
    p.run_meta = runs ? reinterpret_cast<uint32_t *>(d_split + kOffMeta) : nullptr;
    p.run_dump = runs ? w.split_dump.as<uint32_t>() : nullptr;
    p.seg_list = wl.list;
    p.n_seg_ptr = wl.count;
    p.cursor = wl.cursor;
    p.ovf_list = runs || wl.ovf_into >= kTiers ? nullptr : ovf[wl.ovf_into - 1];
    p.ovf_count = d_ctr + CT_OVF1 + wl.ovf_into - 1;  // appended behind what is already there
    // (tiers 6 and 7, whose LDS-array kernels keep arms in HBM: the region named, else their own; the others: tier 6's)
    p.scratch = wl.scratch && tier >= 6 ? wl.scratch : tier == kTiers ? scratch7 : scratch6;
    p.cap_limit = wl.cap_limit;
    p.tier = stat;
    p.seg_slots = w.seg_slots.as<unsigned long long>() + (size_t)4096 * (size_t)(stat & 7);
    p.hb = cx.d_hb ? cx.d_hb + (size_t)2 * SearchCtx::kHbSlots * (size_t)(stat & 7) : nullptr;
    // a workgroup per run; tier 7: as many as its HBM slices (place()).  Option grid<t> may shrink a tier's grid; the
    // workgroup kernels (tiers 3..7) never get more workgroups than their default (HBM scratch is reserved for that many)
    uint64_t g = runs ? n_items : tier == kTiers ? (uint64_t)n_wg7 : (uint64_t)shape(tier).grid;
    if (!runs && opt.grid[tier] > 0) g = tier >= 3 ? std::min<uint64_t>(g, (uint64_t)opt.grid[tier]) : (uint64_t)opt.grid[tier];
    launch_entry(2 * tier + (arms_kernel ? 0 : 1), std::make_integer_sequence<int, 2 * (kTiers + 1)>{}, p,
                 (unsigned)std::min<uint64_t>(n_items, g), st);
    return 0;
}

// the runs over ranges of the cut segments from the work cursor on, one workgroup each, on the main stream (idle while
// the tiers run) -- they are the longest work items of the call.  What a run gives up on is the host's to run again
// (join_ranges): no overflow list, tier 3's count.
template <class SlotT>
int32_t SearchCall<SlotT>::launch_runs(uint32_t n_items) {
    return launch_kernel(0, WorkList{nullptr, reinterpret_cast<const unsigned long long *>(d_split),
                              reinterpret_cast<unsigned long long *>(d_split + 24), Tiers::kRunsTier, test_cap()}, n_items, s);
}

template <class SlotT>
int32_t SearchCall<SlotT>::launch_tier(int tier) {
    if (tier < 1 || tier > kTiers || !n_t[tier - 1]) return 0;
    const int i = tier - 1;
    RC_TRY(launch_kernel(tier, WorkList{order + seg_off[i], d_ctr + CT_N1 + i, d_ctr + CT_CUR1 + i, tier, test_cap()}, n_t[i], tier_stream[tier]));
#ifdef ASGART_PROFILE_EXTEND
    char tag[8];
    snprintf(tag, sizeof tag, "%d", tier);
    PROF_TIER(tag, tier_stream[tier], n_t[tier - 1]);
#endif
    return 0;
}

// tier `tier`'s kernel over the n segments of `list`, on the main stream and with the counters of the re-runs (CT_NF,
// CT_CURF: the previous such launch has been waited for) -- the cascade of finish_tiers, and the cut segments that
// join_ranges runs again as a whole
template <class SlotT>
int32_t SearchCall<SlotT>::rerun_list(int tier, const uint32_t *list, uint64_t n, int ovf_into, uint32_t cap_limit) {
    *h_scalar = n;
    HIP_TRY(hipMemcpyAsync(d_ctr + CT_NF, h_scalar, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_ctr + CT_CURF, 0, 8, s));
    RC_TRY(launch_kernel(tier, WorkList{list, d_ctr + CT_NF, d_ctr + CT_CURF, ovf_into, cap_limit}, n, s));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- every tier and the runs over ranges, launched together; early re-runs of what tiers 3 and 6 give up on ----------------
template <class SlotT>
int32_t SearchCall<SlotT>::run_tiers(int attempt) {
    RC_TRY(w.fam_sds.reserve((size_t)rec_cap * sizeof(SdRec)));
    HIP_TRY(hipMemsetAsync(d_ctr + CT_SD, 0, 8, s));
    HIP_TRY(hipMemsetAsync(d_ctr + CT_NF, 0, (size_t)(CT_COUNT - CT_NF) * 8, s));  // NF, cursors, overflow counts
    HIP_TRY(hipMemsetAsync(d_ctr + CT_EARLY_N, 0, 4 * 8, s));                       // early cascade counts + cursors
    HIP_TRY(hipMemsetAsync(d_ctr + CT_BUSY1, 0, (size_t)(CT_COUNT - CT_BUSY1) * 8, s));
    RC_TRY(w.seg_slots.reserve((size_t)8 * 4096 * 8));
    HIP_TRY(hipMemsetAsync(w.seg_slots.p, 0, (size_t)8 * 4096 * 8, s));
    HIP_TRY(hipEventRecord(cx.ev[EV_TIERS], s));
    base.rp = rp;
    base.p_filt = p_filt;
    base.row_off = row_off;
    base.hits = hits;
    base.recs = w.fam_sds.as<SdRec>();
    base.rec_cap = rec_cap;
    base.escalate_cost = 0xFFFFFFFFu;  // (one-wave tiers: never give up for the work done)
    base.heavy_cap = (uint32_t)heavy_cap64;
    base.solo_hits = opt.solo == 1 ? 16u : (uint32_t)opt.solo;  // (1: the default of 16 hits; other values: that many)
    base.gen_bits = (uint32_t)opt.test_genbits;
    base.k8_delay = (uint32_t)opt.test_k8_delay;
    base.ctr = d_ctr;
    RC_TRY(cx.heartbeat(opt.watchdog_s > 0));
    if (cx.h_hb) memset(cx.h_hb, 0, (size_t)SearchCtx::kHbTiers * SearchCtx::kHbSlots * 16);
    // The tiers are launched together on separate streams, each with a grid that can fill
    // the chip on its own (persistent workgroups, longest segment first): the hardware
    // back-fills CUs as workgroups retire, so the tails of one tier overlap the next.
    // The window bound guarantees that a segment fits its
    // tier, so the overflow lists normally stay empty (they feed the cascade below).
    // Which stream each tier runs on (tier_plan): streams that share a hardware queue run one after the other, so a
    // call has one tier stream per queue it may open, and the tiers that must share a stream are packed by their
    // estimated durations so that no chain outlasts the longest tier by much.
    double est[kTiers + 1];
    plan_estimates(est);
    int32_t stream_of[kTiers], launch_seq[kTiers];
    RC_TRY(tier_plan(cx.n_tier_st, n_t, opt.tier_order, est + 1, n_runs ? est[0] : 0.0, stream_of, launch_seq));
    bool used[SearchCtx::kMaxTierStreams] = {};
    tier_stream[0] = s;
    for (int t = 1; t <= kTiers; ++t) {
        tier_ran[t] = false;
        tier_stream[t] = stream_of[t - 1] > 0 ? cx.tier_st[stream_of[t - 1] - 1] : s;
        if (stream_of[t - 1] > 0) used[stream_of[t - 1] - 1] = true;
    }
    for (int i = 0; i < cx.n_tier_st; ++i)
        if (used[i]) HIP_TRY(hipStreamWaitEvent(cx.tier_st[i], cx.ev[EV_TIERS], 0));
    if (opt.debug) {
        fprintf(stderr, "[asgart] tier plan (%d tier streams; 0 = main stream behind %.1f ms of range runs):", cx.n_tier_st,
                n_runs ? est[0] : 0.0);
        for (int i = 0; i < kTiers && launch_seq[i]; ++i)
            fprintf(stderr, " t%d@%d ~%.1f ms", launch_seq[i], stream_of[launch_seq[i] - 1], est[launch_seq[i]]);
        fprintf(stderr, "\n");
    }
    // Launch order and grid sizes: workgroups are persistent and hold their LDS until the
    // tier's work list is exhausted, so whatever is dispatched first owns the CUs.  The
    // critical path of a pass is the longest tandem-array segment of the heavy tiers
    // (tens of thousands of probes, strictly serial): those tiers go first, the one-wave
    // tier last, and the heavy grids are sized so that every tier's longest segments
    // start at once instead of queueing behind another tier's bulk.
    if (n_runs) {
        // (room for one more run per cut segment: the rest behind the last cut that held, see below)
        RC_TRY(w.split_dump.reserve((size_t)(n_runs + n_splits) * 2 * kRunDumpCap * kDumpWords<SlotT> * 4));
        HIP_TRY(hipMemsetAsync(d_split + 24, 0, 8, s));                         // work cursor
        HIP_TRY(hipMemsetAsync(d_split + kOffMeta, 0, (size_t)n_runs * 64, s));  // run states
        RC_TRY(launch_runs(n_runs));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(cx.runs_ev, s));
    }
    t_launch = std::chrono::steady_clock::now();
    // every tier with work exactly once, in the plan's launch order (tier_plan: the first tier of every stream in the
    // order option tier_order gives, then the second ones; a tier the option leaves out would lose its segments if it
    // never ran); each tier's event follows it on its stream
    for (int i = 0; i < kTiers && launch_seq[i]; ++i) {
        const int t = launch_seq[i];
        RC_TRY(launch_tier(t));
        HIP_TRY(hipEventRecord(cx.tier_ev[t - 1], tier_stream[t]));
        tier_ran[t] = true;
    }
    HIP_TRY(hipGetLastError());
    if (cx.progress && attempt == 0) {
        // Progress (reference src/automaton.rs:98 stores every probe's offset for a polled progress
        // bar): every probe of the call has been searched and its hits are materialised -- the
        // HBM-bound, chip-wide part of the call is over, the extension automaton is under way.
        // A host that pipelines calls (bench.py) issues the next one when it sees this: its search
        // phases then run beside this call's extension, whose tail is a few serial segments.
        if (!progress_given) {
            RC_TRY(wd_event_sync(idx, cx, cx.ev[EV_HIT_ROWS], "the hit rows"));  // probe search, scans and CSR fill are done
            signal_progress();
        }
    }
    // Early cascades of tiers 3 and 6, the two tiers that accept segments above their real capacity (by
    // the allowance): what they give up on need not wait for the other tiers to be re-run -- the longest
    // tier-3 segment of a GRCh38-shaped pass runs 60+ ms longer than tier 6, and in a two-genome run tier 6
    // runs seconds longer than tier 3.  The host waits for whichever of the two finishes first, reads its
    // overflow count and launches the re-run behind it on the same stream; each such launch has its own counters
    // and HBM slices.  The count is read on the main stream, so the re-run cannot start before the runs over
    // ranges -- and any tier the plan put behind them -- have finished (a tier stream would make it wait for the
    // tiers behind this one on that stream instead).
    for (int t = 0; t <= kTiers; ++t) early_n[t] = 0;
    {
        struct Early {
            int src, dst;  // (src's event, cx.tier_ev, follows the re-run on src's stream)
            bool pending;
            char phase[24];  // (what the watchdog names)
        } early[2] = {};  // (two sets of counters, CT_EARLY_N, and of HBM regions, place(); a third tier waits for the cascade)
        int n_early = 0, n_pending = 0;
        unsigned early_polls = 0;
        Watchdog early_wd(idx, cx);
        for (int t = 1; t < kTiers; ++t) {
            if (!shape(t).early || n_early == 2) continue;
            Early &E = early[n_early++];
            E = Early{t, next_holding_more(t), false, {}};
            snprintf(E.phase, sizeof E.phase, "extension tier %d", t);
            // (a re-run in the HBM tier would share that tier's slices with its own list, if it has one; a tier the
            // plan put on the main stream is re-run by the regular cascade: reading its overflow count there would
            // wait for the whole main stream)
            E.pending = n_t[t - 1] && tier_stream[t] != s && (E.dst < kTiers || !n_t[kTiers - 1]);
            n_pending += E.pending ? 1 : 0;
        }
        // (If tier 3's re-run went to tier 6, its kernel would append to tier 6's overflow list while the host
        // snapshots that list's length for tier 6's own early re-run -- a count that may be ahead of the entry:
        // such a re-run waits for the regular cascade below.  With the shipped shapes tier 6 never accepts
        // more than tier 3 and the case does not arise.)
        if (early[0].pending && early[1].pending && early[0].dst == early[1].src) {
            early[0].pending = false;
            --n_pending;
        }
        while (n_pending) {
            bool progressed = false;
            for (int e = 0; e < n_early; ++e) {
                Early &E = early[e];
                if (!E.pending) continue;
                const hipError_t q = hipEventQuery(cx.tier_ev[E.src - 1]);
                if (q == hipErrorNotReady) {
                    (void)hipGetLastError();
                    continue;
                }
                HIP_TRY(q);
                E.pending = false;
                --n_pending;
                progressed = true;
                HIP_TRY(hipMemcpyAsync(h_scalar + 1 + e, d_ctr + CT_OVF1 + E.src - 1, 8, hipMemcpyDeviceToHost, s));
                RC_TRY(wd_sync(idx, cx, s, "an overflow count"));
                const uint64_t n_e = h_scalar[1 + e];
                if (opt.debug)
                    fprintf(stderr, "[asgart] tier %d done %.1f ms after the launches, %llu segment(s) to re-run in tier %d\n",
                            E.src, since_launch(), (unsigned long long)n_e, E.dst);
                if (!n_e) continue;
                early_n[E.src] = n_e;
                // the count the launch works on is fixed now (the list itself may still grow)
                HIP_TRY(hipMemcpyAsync(d_ctr + CT_EARLY_N + e, h_scalar + 1 + e, 8, hipMemcpyHostToDevice, tier_stream[E.src]));
                RC_TRY(launch_kernel(E.dst, WorkList{ovf[E.src - 1], d_ctr + CT_EARLY_N + e, d_ctr + CT_EARLY_CUR + e, E.dst, 0xFFFFFFFFu,
                                                     scratch6 + region * (size_t)(2 + e)}, n_e, tier_stream[E.src]));
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(cx.tier_ev[E.src - 1], tier_stream[E.src]));
            }
            if (n_pending && !progressed) {
                std::this_thread::sleep_for(std::chrono::microseconds(50));
                // (the same watchdog as every other wait of the call -- one look at the heartbeats, never a blocking
                // wait: the other tier's early re-run must not wait for this one's stream to drain)
                if ((++early_polls & 0x3FFu) == 0 && early_wd.expired(early[early[0].pending ? 0 : 1].phase)) return ASGART_E_HIP;
            }
        }
    }
    return 0;
}

// ---- statistics of the tiers; the cascade: what tier t gave up on is re-run by the next tier that holds more ------------------
template <class SlotT>
int32_t SearchCall<SlotT>::finish_tiers() {
    PROF_DUMP("concurrent tiers");
    if (opt.debug) {
        fprintf(stderr, "[asgart] all tiers and early re-runs done %.1f ms after the launches\n", since_launch());
        // how much of the chip each tier held: sum of its workgroups' lifetimes x the share of a compute unit one of
        // them occupies
        double tot = 0.0;
        fprintf(stderr, "[asgart] compute-unit time held per tier (CU-ms; workgroups):");
        for (int t = 1; t <= kTiers; ++t) {
            const double cu_ms = (double)tier_sum(CT_BUSY1, t) * 1e-5 / stat_shape(t).wg_per_cu;
            tot += cu_ms;
            fprintf(stderr, " %d: %.0f (%llu)", t, cu_ms, tier_sum(CT_WGS1, t));
        }
        fprintf(stderr, "  total %.0f = %.1f ms of the whole chip\n", tot, tot / 256.0);
        fprintf(stderr, "[asgart] per tier: hit-probes / hits per hit-probe / CU-microseconds per hit-probe:");
        for (int t = 1; t <= kTiers; ++t) {
            const double hp = (double)h_tp[t - 1];
            fprintf(stderr, " %d: %.0fK / %.1f / %.2f", t, hp / 1e3, hp > 0 ? (double)h_th[t - 1] / hp : 0.0,
                    hp > 0 ? (double)tier_sum(CT_BUSY1, t) * 1e-2 / stat_shape(t).wg_per_cu / hp : 0.0);
        }
        fprintf(stderr, "\n");
    }
    {   // the longest chain of tiers on one stream (early re-runs included): the serial floor of this call's extension
        float longest = 0.f;
        for (int t = 1; t <= kTiers; ++t) {
            float ms = 0.f;
            if (!tier_ran[t]) continue;
            if (hipEventElapsedTime(&ms, cx.ev[EV_TIERS], cx.tier_ev[t - 1]) == hipSuccess) longest = std::max(longest, ms);
            else (void)hipGetLastError();
        }
        ms_longest_tier = longest;
    }
    n_overflow = 0;
    for (int t = 1; t < kTiers; ++t) n_overflow += h_ctr[CT_OVF1 + t - 1];
    if (opt.debug) {
        fprintf(stderr, "[asgart] overflow out of tiers 1..%d:", kTiers - 1);
        for (int t = 1; t < kTiers; ++t) fprintf(stderr, " %llu", (unsigned long long)h_ctr[CT_OVF1 + t - 1]);
        fprintf(stderr, "\n");
    }
    n_heavy = 0;
    for (int t = 3; t <= kTiers; ++t) n_heavy += n_t[t - 1];
    // ---- cascade: what tier t gave up on is re-run from its start by the next tier that
    // is in use and holds more arms (its own overflow is appended to that tier's list) ------
    const auto t_casc0 = std::chrono::steady_clock::now();
    for (int src = 1; src < kTiers; ++src) {
        // (the first early_n entries of the list have been re-run already; a lower tier's cascade into
        // this tier may have appended more)
        const uint64_t skip = early_n[src];
        const uint64_t n_ovf = h_ctr[CT_OVF1 + src - 1] - skip;
        if (!n_ovf) continue;
        const int dst = next_holding_more(src);
        RC_TRY(rerun_list(dst, ovf[src - 1] + skip, n_ovf, dst, 0xFFFFFFFFu));
        HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, kCtrBytes, hipMemcpyDeviceToHost, s));
        RC_TRY(wd_sync(idx, cx, s, "a re-run of overflowed segments"));
        PROF_DUMP("cascade");
    }
    ms_tier2 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() -
                                                         t_casc0).count();
    if (h_ctr[CT_OVF1 + kTiers - 1]) {
        // (cannot happen: tier 7 holds the bound on the live arms of any segment -- unless a test shrank it)
        set_error("internal: %llu segment(s) overflowed the last extension tier (%llu arm slots)",
                  (unsigned long long)h_ctr[CT_OVF1 + kTiers - 1], (unsigned long long)heavy_cap64);
        return ASGART_E_CAP;
    }
    ms_longest_segment = 0.0;
    for (int t = 0; t < kRunsStat; ++t) ms_longest_segment = std::max(ms_longest_segment, (double)h_ctr[CT_SEGMAX1 + t] * 1e-5);
    if (opt.debug) {
        fprintf(stderr, "[asgart] longest single segment per tier (ms):");
        for (int t = 1; t <= kTiers; ++t) fprintf(stderr, " %d: %.2f", t, (double)tier_longest(t) * 1e-5);
        fprintf(stderr, "\n");
    }
#ifdef ASGART_SEG_TOP
    if (opt.debug) {  // diagnostic build: the 48 longest segments per tier (seg_clock's log)
        std::vector<unsigned long long> log(4096);
        HIP_TRY(hipMemcpy(log.data(), w.seg_slots.as<unsigned long long>() + 4096, log.size() * 8, hipMemcpyDeviceToHost));
        for (int stat = 2; stat <= kRunsStat; ++stat) {
            unsigned long long *l = log.data() + (size_t)kSegTopWords * (stat & 7);
            const size_t n_log = (size_t)std::min<unsigned long long>(l[0], kSegTopWords - 1);
            std::sort(l + 1, l + 1 + n_log, std::greater<unsigned long long>());
            fprintf(stderr, "[asgart] %s%d: %llu segments of %.1f ms and more; the longest (ms):", stat == kRunsStat ? "runs, as tier " : "tier ",
                    stat == kRunsStat ? Tiers::kRunsTier : stat, l[0], (double)kSegTopMin * 1e-5);
            for (size_t i = 0; i < std::min<size_t>(n_log, 48); ++i) fprintf(stderr, " %.2f", (double)l[1 + i] * 1e-5);
            fprintf(stderr, "\n");
        }
    }
#endif
    remember_plan_estimates();
    return 0;
}

// ---- the estimates of the tier plan (tier_plan) ---------------------------------------------------------------------------
// est[t]: tier t's estimated duration in ms, est[0]: the runs over ranges -- what the previous call with the same
// call_sig measured (remember_plan_estimates), else the table's profile
// (what remembered estimates belong to: the call's settings and chunks, and the thresholds its placement moved tails by)
template <class SlotT>
uint64_t SearchCall<SlotT>::plan_sig() const {
    uint64_t sig = call_sig;
    for (int t = 1; t <= kTiers; ++t) sig = (sig ^ tail_hits[t]) * 1099511628211ull;
    return sig;
}
template <class SlotT>
void SearchCall<SlotT>::plan_estimates(double *est) const {
    const bool known = cx.plan_known && cx.plan_sig == plan_sig();
    for (int t = 0; t <= kTiers; ++t) {
        const TierShape &sh = stat_shape(t);
        // (a tier whose tail this call moved away: the profile's figure for what is left of it)
        const double profile = tail_hits[t] && sh.tail_hits && sh.tail_profile_ms > 0.0 ? sh.tail_profile_ms : sh.profile_ms;
        est[t] = known && cx.plan_est[t] > 0.0 ? cx.plan_est[t] : profile;
    }
}
// per tier that ran: the longer of its longest segment and its work spread over the compute units its default grid can
// hold -- tier 1's 2048 one-wave workgroups fill 186 of them, the others the whole chip (the runs over ranges have a
// statistics slot of their own, kRunsStat, and their own estimate: their duration, est[0])
template <class SlotT>
void SearchCall<SlotT>::remember_plan_estimates() {
    if (!(cx.plan_known && cx.plan_sig == plan_sig()))
        for (double &e : cx.plan_est) e = 0.0;
    cx.plan_sig = plan_sig();
    cx.plan_known = true;
    for (int t = 1; t <= kTiers; ++t) {
        if (!tier_ran[t]) continue;
        const double seg = (double)h_ctr[CT_SEGMAX1 + t - 1] * 1e-5;
        const TierShape &sh = stat_shape(t);
        const double spread = (double)h_ctr[CT_BUSY1 + t - 1] * 1e-5 / sh.wg_per_cu / std::min(256.0, (double)sh.grid / sh.wg_per_cu);
        cx.plan_est[t] = std::max(seg, spread);
    }
    float runs = 0.f;
    if (n_runs) {
        if (hipEventElapsedTime(&runs, cx.ev[EV_TIERS], cx.runs_ev) != hipSuccess) {
            (void)hipGetLastError();
            runs = 0.f;
        }
        cx.plan_est[0] = runs;
    }
    // The launches whose workgroups hold whole compute units (tier 3, tier 6, tier 7, the runs) get a unit only when
    // nothing else is left on it, and a GRCh38-shaped step is bound by compute-unit time: such a launch does not end
    // before the chip has served the compute-unit time of everything that starts with it, however short its own
    // longest segment (tier 6: 33.6 ms of longest segment, 36 ms of whole-unit work spread over the chip, traced at
    // 0-59 ms beside the other tiers, whose 14.4 CU-seconds are 56 ms of the chip).
    double chip_ms = 0.0;
    auto ran = [&](int t) { return t ? tier_ran[t] : n_runs != 0; };
    for (int t = 0; t <= kTiers; ++t)
        if (ran(t)) chip_ms += (double)h_ctr[CT_BUSY1 + (t ? t : kRunsStat) - 1] * 1e-5 / stat_shape(t).wg_per_cu / 256.0;
    for (int t = 0; t <= kTiers; ++t)
        if (ran(t) && stat_shape(t).wg_per_cu == 1) cx.plan_est[t] = std::max(cx.plan_est[t], chip_ms);
}

}  // namespace asgart
