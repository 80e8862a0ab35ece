// call_place.hpp -- stage place of a search call.
// Part of pipeline.hip, the one translation unit that launches the search kernels (search_call.hpp has the stage list).
#pragma once
#include "search_call.hpp"

namespace asgart {

// ---- placement: per-segment work estimate -> tier, longest first; barren segments; long segments as ranges ----------------
template <class SlotT>
int32_t SearchCall<SlotT>::place() {
    rec_cap = std::max<uint64_t>(1u << 18, w.fam_sds.cap / sizeof(SdRec));
    RC_TRY(w.ovf_list.reserve((size_t)(n_seg + 1) * 4 * kTiers));
    h_recs = nullptr;
    n_hrec = 0;
    // ---- placement: per-segment work estimate -> tier, longest first --------------------
    // option force_tier = t (tests): start every segment with a multi-hit probe in tier >= t
    const int force_tier = (int)opt.force_tier;
    RC_TRY(w.seg_keys.reserve((size_t)n_seg * 4 * 2));
    RC_TRY(w.seg_vals.reserve((size_t)n_seg * 4 * 2));
    uint32_t *kbuf = w.seg_keys.as<uint32_t>(), *vbuf = w.seg_vals.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_ctr + CT_N1, 0, (size_t)(CT_COUNT - CT_N1) * 8, s));
    // ---- the tiers (TierTable): what each accepts ---------------------------------------------
    arms_kernel = rp.C <= (uint64_t)kHitBatch && opt.arms_kernel != 0 && (uint64_t)idx->n < (1ull << 42);
    for (int t = 1; t <= kTiers; ++t) {
        const TierShape &sh = shape(t);
        // (an arm-resident shape stages the whole hit row of a probe: it is skipped when max_cardinality exceeds that)
        const bool usable = sh.kernel != TierKernel::none && !(arms_kernel && rp.C > (uint64_t)sh.hits);
        tier_cap[t] = usable ? (uint32_t)((uint64_t)sh.cap() * (uint64_t)(sh.widen ? opt.*sh.widen : 100) / 100u) : 0u;
    }
    tier_cap[kTiers] = 0xFFFFFFFFu;  // (tier 7 takes whatever is left)
    if (arms_kernel)  // (tier 3: what tier 6 accepts, within its own allowance)
        tier_cap[3] = std::min(std::max(shape(3).cap(), tier_cap[6]), tier_cap[3]);
    else              // (the hybrid kernel: 40 % over by the bound as well; 16-bit gap / pend)
        tier_cap[6] = (rp.G >= 0xFFF0u || rp.C >= 0xFFF0u) ? 0u : tier_cap[6] * 7 / 5;
    PlaceParams pp;
    pp.long3 = pp.long3_big = pp.dense3 = pp.dense6 = 0;
    pp.stats = opt.debug ? 1u : 0u;
    pp.barren = opt.barren ? 1u : 0u;
    pp.seg_info = nullptr;
    const bool cluster_barren = opt.barren >= 2 && rp.M > (uint64_t)k;
    // long segments as ranges side by side (option split; plan_ranges_kernel in ranges_dev.hpp): the long shape of the
    // one-barrier kernel; also in a sharded call (the segments its window cuts short are left alone: only
    // a segment whose end the placement walk has seen is cut)
    split_on = opt.split >= (sizeof(SlotT) == 4 ? 1 : 2) && arms_kernel && (opt.split_len == 0 || opt.split_len >= 64);
    if (cluster_barren || split_on) {
        RC_TRY(w.seg_info.reserve((size_t)n_seg * sizeof(uint2)));
        pp.seg_info = w.seg_info.as<uint2>();
    }
    d_split = nullptr;
    if (split_on) {
        RC_TRY(w.split_buf.reserve(kSplitBytes));
        d_split = w.split_buf.as<char>();
        HIP_TRY(hipMemsetAsync(d_split, 0, 64, s));
    }
    pp.k = (uint32_t)k;
    pp.step = (uint32_t)step;
    pp.G = rp.G;
    pp.M = rp.M;
    for (int t = 1; t < kTiers; ++t) pp.cap[t - 1] = tier_cap[t];
    if (arms_kernel) {
        pp.long3 = (uint32_t)opt.long3;
        pp.long3_big = pp.long3 / 4u;
        pp.dense3 = (uint32_t)opt.dense3;
        pp.dense6 = (uint32_t)opt.dense6;
        if (force_tier == 3) {
            pp.long3 = pp.long3_big = 1;
            pp.dense3 = pp.dense6 = 0;
        }
        pp.cap[0] = (uint32_t)std::min<int64_t>(opt.cap1, shape(1).cap());
    }
    {   // the tail rule (place_tier): by default only where tiers must share a stream -- with a stream per arm-resident
        // tier every launch lasts as long as its own longest segment and nothing waits behind it
        int n_resident = 0;
        for (int t = 2; t < kTiers; ++t)
            n_resident += tier_enabled(t) && (shape(t).kernel == TierKernel::fast || shape(t).kernel == TierKernel::k8) ? 1 : 0;
        const bool on = tail_up.mode == 2 || (tail_up.mode == 1 && cx.n_tier_st < n_resident);
        for (int t = 1; t < kTiers; ++t) {
            // (arm-resident shapes only: the LDS-array set keeps its segments whatever the settings)
            const bool source = (t == 2 || t == 4 || t == 5) && shape(t).kernel == TierKernel::fast;
            const uint32_t thr = !source ? 0u : tail_up.hits > 0 ? (uint32_t)std::min<int64_t>(tail_up.hits, 0xFFFFFFFFll) : shape(t).tail_hits;
            pp.tail_hits[t - 1] = tail_hits[t] = on && tier_enabled(t) ? thr : 0u;
        }
    }
    int force_eff = force_tier;  // a forced tier that has no kernel in this mode: the next one that has
    while (force_eff > 1 && force_eff < kTiers && !tier_enabled(force_eff)) ++force_eff;
    pp.sum1 = kTier1MaxSum;
    pp.force_tier = force_eff;
    {
        // one segment per lane for the first kLaneWalk probes, the longer ones wave by wave (their list
        // borrows the overflow lists' buffer, which the tiers only use afterwards)
        uint32_t *long_list = w.ovf_list.as<uint32_t>();
        seg_stats_lanes_kernel<<<(unsigned)std::min<uint64_t>((n_seg + 63) / 64, 256ull * 9ull * 2ull), 64, 0, s>>>(
            rp, p_filt, seg_list, d_ctr + CT_SEG, kbuf, vbuf, pp, long_list, d_ctr);
        seg_stats_kernel<<<(unsigned)std::min<uint64_t>(n_seg, 256ull * 16ull), 64, 0, s>>>(
            rp, p_filt, seg_list, d_ctr + CT_LONGSEG, long_list, kbuf, vbuf, pp, d_ctr);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamWaitEvent(s, cx.ev[EV_HIT_ROWS], 0));  // the hit rows (front(): filled beside the walk above)
    if (cluster_barren) {
        HIP_TRY(hipEventRecord(cx.ev[EV_BARREN], s));
        // barren by position (cluster_barren_kernel): a wave per segment, two bitmap sizes (2 KB: 32 waves per compute
        // unit; 16 KB: 9)
        cluster_barren_kernel<SlotT, 16384><<<256 * 32, 64, 0, s>>>(rp, pp, row_off, hits, seg_list, d_ctr + CT_SEG, kbuf, 1u, 1024u,
                                                                   d_ctr + CT_CLUSTER_CUR, d_ctr);
        HIP_TRY(hipEventRecord(cx.ev[EV_BARREN_SMALL], s));
        cluster_barren_kernel<SlotT, 131072><<<256 * 9, 64, 0, s>>>(rp, pp, row_off, hits, seg_list, d_ctr + CT_SEG, kbuf, 1025u,
                                                                   16384u, d_ctr + CT_CLUSTER_CUR + 1, d_ctr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(cx.ev[EV_BARREN_BIG], s));
    }
    if (split_on) {
        SplitParams sp{};
        sp.range_len = (uint32_t)opt.split_len;
        sp.warm = (uint32_t)opt.split_warm;
        sp.min_span = (uint32_t)std::min<int64_t>(opt.split_min, 0x7FFFFFFF);
        sp.max_runs = kMaxRuns - kMaxSplits;  // (one more run per cut segment may follow)
        sp.max_cuts = kMaxCuts;
        sp.max_splits = kMaxSplits;
        {   // segments a cut of which failed in an earlier call of this index with these settings and chunks, if this
            // call's windows hold them: as probe numbers of THIS call (the newest verdicts first)
            // (blocked_in_call, range_join.hpp: next to what join_ranges remembers)
            BlockedSeg *h_blocked = reinterpret_cast<BlockedSeg *>(h_split + kOffBlocked);
            std::lock_guard<std::mutex> lk(idx->mu);
            sp.n_blocked = blocked_in_call(idx->split_blocked, call_sig, rp.modes, n_passes, lo_lim, hi_lim, kSplitBlockedMax,
                                           [&](int32_t p_, const SplitVerdict &b) {
                                               *h_blocked++ = BlockedSeg{(uint32_t)p_ * K + ((uint32_t)b.key - lo_lim), b.range_len, b.allowed, b.warm};
                                           });
        }
        sp.blocked = reinterpret_cast<const BlockedSeg *>(d_split + kOffBlocked);
        if (sp.n_blocked)
            HIP_TRY(hipMemcpyAsync(d_split + kOffBlocked, h_split + kOffBlocked, (size_t)sp.n_blocked * sizeof(BlockedSeg), hipMemcpyHostToDevice, s));
        SplitChoice *const d_choice = reinterpret_cast<SplitChoice *>(d_split + kOffChoice);
        if (!sp.range_len) {  // the range length by budget
            HIP_TRY(hipMemsetAsync(d_choice, 0, sizeof(SplitChoice), s));
            split_tally_kernel<<<grid_for(n_seg), 256, 0, s>>>(rp, d_ctr + CT_SEG, kbuf, pp.seg_info, d_choice);
            split_pick_kernel<<<1, 1, 0, s>>>(d_choice, (uint32_t)opt.split_runs);
        }
        plan_ranges_kernel<<<grid_for(n_seg), 256, 0, s>>>(rp, sp, p_filt, seg_list, d_ctr + CT_SEG, kbuf, pp.seg_info,
                                                          reinterpret_cast<unsigned long long *>(d_split),
                                                          reinterpret_cast<RangeRun *>(d_split + kOffRuns),
                                                          reinterpret_cast<uint2 *>(d_split + kOffCuts),
                                                          reinterpret_cast<SplitSeg *>(d_split + kOffSplits), d_choice);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_split, d_split, kOffMeta, hipMemcpyDeviceToHost, s));
    }
    if (opt.debug >= 2 && pp.seg_info) {  // the longest and the richest segment every tier runs WHOLE
        unsigned long long *d_top = nullptr, h_top[2 * kTiers] = {};
        HIP_TRY(hipMalloc(&d_top, sizeof(h_top)));
        (void)hipMemsetAsync(d_top, 0, sizeof(h_top), s);
        top_uncut_kernel<<<grid_for(n_seg), 256, 0, s>>>(d_ctr + CT_SEG, kbuf, pp.seg_info, d_top);
        (void)hipMemcpyAsync(h_top, d_top, sizeof(h_top), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        for (int t = 0; t < 2 * kTiers; ++t) {
            if (!h_top[t]) continue;
            uint2 info{};
            uint32_t g0 = 0;
            const size_t sj = (size_t)(h_top[t] & 0xFFFFFFFFull);
            (void)hipMemcpy(&info, pp.seg_info + sj, sizeof(info), hipMemcpyDeviceToHost);
            (void)hipMemcpy(&g0, seg_list + sj, sizeof(g0), hipMemcpyDeviceToHost);
            fprintf(stderr, "[asgart] tier %d, run whole, the segment with the most %s: at probe %u, %u probe positions%s, %u hits\n", t / 2 + 1,
                    t % 2 ? "hits" : "probe positions", g0, info.y & 0x7FFFFFFFu, (info.y >> 31) ? "" : " (cut short by the window)", info.x);
        }
        (void)hipFree(d_top);
        // ... and the hit totals of the 48 richest segments every tier runs whole (its list is sorted by them: they start first)
        std::vector<uint32_t> h_keys((size_t)n_seg);
        std::vector<uint2> h_info((size_t)n_seg);
        (void)hipMemcpy(h_keys.data(), kbuf, (size_t)n_seg * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(h_info.data(), pp.seg_info, (size_t)n_seg * sizeof(uint2), hipMemcpyDeviceToHost);
        for (uint32_t t = 1; t < (uint32_t)kTiers; ++t) {
            std::vector<uint32_t> rich;
            for (size_t sj = 0; sj < (size_t)n_seg; ++sj)
                if (h_keys[sj] >> 29 == t) rich.push_back(h_info[sj].x);
            const size_t top = std::min<size_t>(rich.size(), 48);
            std::partial_sort(rich.begin(), rich.begin() + top, rich.end(), std::greater<uint32_t>());
            fprintf(stderr, "[asgart] tier %u, run whole, the most hits:", t + 1);
            for (size_t i = 0; i < top; ++i) fprintf(stderr, " %u", rich[i]);
            fprintf(stderr, "\n");
        }
    }
    order = nullptr;
    const uint32_t *sorted_keys = nullptr;
    RC_TRY(sort_segments(w, kbuf, vbuf, n_seg, s, &order, &sorted_keys, false));
    tier_bounds_kernel<<<1, 64, 0, s>>>(sorted_keys, d_ctr + CT_SEG, d_ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, kCtrBytes, hipMemcpyDeviceToHost, s));
    RC_TRY(wd_sync(idx, cx, s, "the hit rows and the placement of the segments"));
    seg_off[0] = 0;
    for (int t = 0; t < kTiers; ++t) {
        n_t[t] = h_ctr[CT_N1 + t];
        seg_off[t + 1] = seg_off[t] + n_t[t];
        h_tp[t] = h_ctr[CT_TPROBES1 + t];
        h_th[t] = h_ctr[CT_THITS1 + t];
        cx.tier_segments[t] = n_t[t];
    }
    cx.tier_segments[kTiers] = h_ctr[CT_TAIL_UP];
    h_split_hdr = reinterpret_cast<const unsigned long long *>(h_split);
    n_runs = split_on ? (uint32_t)h_split_hdr[0] : 0u;
    n_cuts = split_on ? (uint32_t)h_split_hdr[1] : 0u;
    n_splits = split_on ? (uint32_t)h_split_hdr[2] : 0u;
    split_segs.assign(n_splits, SplitSeg{});
    if (n_splits) memcpy(split_segs.data(), h_split + kOffSplits, (size_t)n_splits * sizeof(SplitSeg));
    n_split_segments = n_splits;
    if (opt.debug && split_on)
        for (const SplitSeg &sg : split_segs)
            fprintf(stderr, "[asgart] ranges: segment at probe %u: tier %u, %u probe positions, %u hits -> %u ranges\n", sg.g_seg0, sg.tier, sg.span,
                    sg.hits, sg.n_ranges);
    if (opt.debug && split_on)
        fprintf(stderr, "[asgart] %u long segment(s) cut into ranges: %u runs (ranges of %llu probes%s), %u cuts to check\n",
                n_splits, n_runs, (unsigned long long)h_split_hdr[4], opt.split_len ? "" : ": the shortest that keeps the runs within the budget", n_cuts);
    if (opt.debug) {
        fprintf(stderr, "[asgart] %llu segments, %llu walked wave by wave; per tier:", (unsigned long long)n_seg,
                (unsigned long long)h_ctr[CT_LONGSEG]);
        unsigned long long placed = 0;
        for (int t = 0; t < kTiers; ++t) {
            fprintf(stderr, " %llu", (unsigned long long)n_t[t]);
            placed += n_t[t];
        }
        fprintf(stderr, "; %llu barren (no arm can reach min_duplication_length: not run), %llu of them by the positions of their hits\n",
                (unsigned long long)n_seg - placed, (unsigned long long)h_ctr[CT_CLUSTER_BARREN]);
        fprintf(stderr, "[asgart] tail rule: thresholds (hits) of tiers 2, 4, 5: %u %u %u; %llu segment(s) moved to the next tier that holds more\n",
                pp.tail_hits[1], pp.tail_hits[3], pp.tail_hits[4], (unsigned long long)h_ctr[CT_TAIL_UP]);
        if (cluster_barren) {
            float ms_a = 0.f, ms_b = 0.f, ms_p = 0.f;
            (void)hipEventElapsedTime(&ms_a, cx.ev[EV_BARREN], cx.ev[EV_BARREN_SMALL]);
            (void)hipEventElapsedTime(&ms_b, cx.ev[EV_BARREN_SMALL], cx.ev[EV_BARREN_BIG]);
            (void)hipEventElapsedTime(&ms_p, cx.ev[EV_FILL], cx.ev[EV_BARREN]);
            fprintf(stderr, "[asgart] hit rows filled, placement walk beside it: %.2f ms; barren by position: segments of up to 1 024 hits %.2f ms, up to 16 384 hits %.2f ms\n",
                    ms_p, ms_a, ms_b);
        }
    }
    for (int t = 0; t < kTiers; ++t) ovf[t] = w.ovf_list.as<uint32_t>() + (size_t)t * (n_seg + 1);
    // HBM arm storage of the LDS-array kernels: tier 6 (MODE 1) and tier 7 (MODE 2) may run at the
    // same time on different streams, so each gets its own region of 256 per-workgroup slices
    // Tier 7 never refuses a segment for its size: max_cardinality * (t* + 1) bounds the live arms of ANY segment
    // (every live arm was created or extended within the last t* + 1 processed probes, at most max_cardinality
    // per probe; src/automaton.rs:87 keeps them in an unbounded Vec), and its slices are sized for that.  Large
    // bounds get fewer workgroups (a 16 GB budget for the four regions), never fewer than one.
    // (rounded up to a multiple of 4: a workgroup's slice holds 64-bit position arrays behind arrays of this many
    // 32-bit words, and slices, regions and the early-cascade regions follow one another at multiples of it)
    heavy_cap64 = (std::max<uint64_t>((uint64_t)rp.C * ((uint64_t)rp.tstar + 1u) + 64u, 4096u) + 3u) & ~3ull;
    if (heavy_cap64 >= (1ull << 24)) {
        set_error("max_cardinality * (max_gap_size / step + 1) = %llu live arms per segment: more than 2^24 are not supported",
                  (unsigned long long)heavy_cap64);
        return ASGART_E_CAP;
    }
    const size_t per_wg7 = (size_t)heavy_cap64 * (4 * sizeof(SlotT) + 28);
    const size_t per_wg6 = (size_t)caph * (4 * sizeof(SlotT) + 16);
    const size_t per_wg = std::max(per_wg6, per_wg7);
    n_wg7 = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(256, (16ull << 30) / (4 * per_wg)));
    region = std::max(per_wg6 * 256, per_wg * (size_t)n_wg7);  // (a region serves either kind of launch)
    RC_TRY(w.scratch.reserve(region * 4));  // tier 6, tier 7, and one region per early cascade launch
    scratch6 = w.scratch.as<char>();
    scratch7 = scratch6 + region;
    return 0;
}

}  // namespace asgart
