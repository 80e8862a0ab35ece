// call_join.hpp -- stage join_ranges of a search call; the rules it applies are range_join.hpp's.
// Part of pipeline.hip, the one translation unit that launches the search kernels (search_call.hpp has the stage list).
#pragma once
#include "search_call.hpp"

namespace asgart {

static_assert(kPlanAllCuts == kAllCuts, "range_join.hpp restates BlockedSeg's every-cut mark");

// the fix table (h_split + kOffFix) to the device, and the records' family ordinals through it
template <class SlotT>
int32_t SearchCall<SlotT>::apply_fix() {
    HIP_TRY(hipMemcpyAsync(d_split + kOffFix, h_split + kOffFix, kOffAgain - kOffFix, hipMemcpyHostToDevice, s));
    const uint64_t n_slots = std::min<uint64_t>(h_ctr[CT_SD], rec_cap);
    if (n_slots) fixup_records_kernel<<<grid_for(n_slots), 256, 0, s>>>(w.fam_sds.as<SdRec>(), n_slots, reinterpret_cast<const uint32_t *>(d_split + kOffFix));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the tiers are through: cuts checked, ranges joined up, refused segments run again --------------------------------------
template <class SlotT>
int32_t SearchCall<SlotT>::join_ranges() {
    for (int t = 1; t <= kTiers; ++t)
        if (tier_ran[t] && tier_stream[t] != s) HIP_TRY(hipStreamWaitEvent(s, cx.tier_ev[t - 1], 0));
    if (n_cuts) {
        validate_cuts_kernel<kDumpWords<SlotT>><<<n_cuts, 256, 0, s>>>(reinterpret_cast<const uint2 *>(d_split + kOffCuts),
                                                   reinterpret_cast<const uint32_t *>(d_split + kOffMeta), w.split_dump.as<uint32_t>(),
                                                   reinterpret_cast<uint32_t *>(d_split + kOffOk));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_split + kOffMeta, d_split + kOffMeta, kOffFix - kOffMeta, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, kCtrBytes, hipMemcpyDeviceToHost, s));
    RC_TRY(wd_sync(idx, cx, s, "the extension tiers"));
    if (n_runs) {
        // What stands of a segment a cut of which did not hold, and what runs again: join_segment and settle_tail
        // (range_join.hpp).  The index remembers what the segment needs from then on (remember, below): a longer warm-up, or
        // only the cuts that held.
        const uint32_t *h_meta = reinterpret_cast<const uint32_t *>(h_split + kOffMeta);
        const uint32_t *h_ok = reinterpret_cast<const uint32_t *>(h_split + kOffOk);
        RangeRun *h_runs = reinterpret_cast<RangeRun *>(h_split + kOffRuns);
        uint32_t *h_fix = reinterpret_cast<uint32_t *>(h_split + kOffFix);
        uint32_t *h_again = reinterpret_cast<uint32_t *>(h_split + kOffAgain);
        uint32_t n_again = 0, n_tail = 0;
        n_split_refused = 0;
        struct Tail {
            uint32_t run, base, g_seg0, run_base, f;
            size_t held_at;  // its ranges' bases in held_base
        };
        std::vector<uint32_t> held_base;  // family-ordinal bases of the ranges whose records wait for their segment's last run
        std::vector<Tail> tails;
        // (split_warm_next and remember_split, range_join.hpp, say what is remembered and why)
        auto remember = [&](uint32_t g_seg0, uint32_t allowed, uint32_t warm_used, uint32_t need) {
            const uint32_t p_ = pass_of_probe(g_seg0);
            const uint64_t key_ = (uint64_t)((rp.modes >> (8 * p_)) & 0xFFu) << 32 | (uint64_t)pass_offset(g_seg0);
            const uint32_t len_ = (uint32_t)h_split_hdr[4];
            const uint32_t warm_next = split_warm_next(warm_used, need, len_, (uint64_t)opt.split_warm_max);
            std::lock_guard<std::mutex> lk(idx->mu);
            remember_split(idx->split_blocked, key_, call_sig, len_, allowed, warm_next);
        };
        for (const SplitSeg &sg : split_segs) {
            const uint32_t n_cuts_sg = sg.n_ranges - 1;
            const bool last_gave_up = h_meta[(size_t)(sg.run_base + sg.n_ranges - 1) * 16 + 4] != 0u;
            const size_t held_at = held_base.size();
            held_base.resize(held_at + sg.n_ranges);
            const JoinVerdict jv = join_segment(sg.n_ranges, h_ok + sg.cut_base, h_meta + (size_t)sg.run_base * 16 + 1, 16, last_gave_up,
                                                h_fix + sg.run_base, held_base.data() + held_at);
            const uint32_t f = jv.f;
            const bool ok = jv.action == JoinAction::joined;
            held_base.resize(held_at + (jv.action == JoinAction::tail_run ? f + 1 : 0));
            if (jv.action == JoinAction::tail_run) {
                RangeRun t = h_runs[sg.run_base + f];
                t.g_stop = 0xFFFFFFFFu;
                t.emit_from = h_runs[sg.run_base + f + 1].emit_from;
                t.flags = kRunLast;
                h_runs[n_runs + n_tail] = t;
                tails.push_back(Tail{n_runs + n_tail, jv.tail_base, sg.g_seg0, sg.run_base, f, held_at});
                ++n_tail;
            }
            if (!ok && opt.debug) {
                fprintf(stderr, "[asgart] ranges: segment at probe %u (%u ranges): %u cut(s) held; cuts (arms in the range in front / in the range behind, family open, held flush):",
                        sg.g_seg0, sg.n_ranges, f);
                for (uint32_t j = 0; j < n_cuts_sg; ++j) {
                    const uint32_t *ma = h_meta + (size_t)(sg.run_base + j) * 16, *mb = h_meta + (size_t)(sg.run_base + j + 1) * 16 + 8;
                    fprintf(stderr, " %s%u/%u,%u/%u,%u/%u%s", (h_ok[sg.cut_base + j] & 1u) ? "" : "[", ma[0], mb[0], ma[2], mb[2], ma[3], mb[3],
                            (h_ok[sg.cut_base + j] & 1u) ? "" : "]");
                }
                fprintf(stderr, "%s\n", last_gave_up ? " (the last range gave up)" : "");
            }
            if (!ok) {
                ++n_split_refused;
                uint32_t need = 0;  // probes between the birth of the oldest arm in front of the failed cut and that cut
                if (f < n_cuts_sg) {
                    const uint32_t born = (h_ok[sg.cut_base + f] >> 1) / (uint32_t)rp.step, at = h_runs[sg.run_base + f + 1].emit_from - sg.g_seg0;
                    if ((h_ok[sg.cut_base + f] >> 1) != (0xFFFFFFFFu >> 10) && born <= at) need = at - born;
                }
                if (opt.debug)
                    fprintf(stderr, "[asgart] ranges: segment at probe %u: cut %u did not hold with %u probes of warm-up; its oldest arm was born %u probes in front of it\n",
                            sg.g_seg0, f, sg.warm, need);
                remember(sg.g_seg0, f, last_gave_up ? 0u : sg.warm, need);
                if (f == 0) h_again[n_again++] = sg.g_seg0;
            }
        }
        if (opt.debug) {  // the runs' durations, per cut segment (ms)
            for (const SplitSeg &sg : split_segs) {
                fprintf(stderr, "[asgart] ranges: segment at probe %u (tier %u, %u positions, %u hits): runs", sg.g_seg0, sg.tier, sg.span, sg.hits);
                for (uint32_t j = 0; j < sg.n_ranges; ++j) fprintf(stderr, " %.1f", (double)h_meta[(size_t)(sg.run_base + j) * 16 + 5] * 1e-5);
                fprintf(stderr, " ms\n");
            }
        }
        if (opt.debug)
            fprintf(stderr, "[asgart] ranges: %llu of %u cut segment(s) joined up%s\n", (unsigned long long)(n_splits - n_split_refused), n_splits,
                    n_split_refused ? "; the others: the rest behind the last cut that held as one more run, or the whole segment again" : "");
        for (const Tail &t : tails) h_fix[t.run] = kFixHeld;  // (until the run has come back)
        RC_TRY(apply_fix());
        if (n_tail) {
            HIP_TRY(hipMemcpyAsync(d_split + kOffRuns + (size_t)n_runs * sizeof(RangeRun), h_runs + n_runs, (size_t)n_tail * sizeof(RangeRun),
                                   hipMemcpyHostToDevice, s));
            h_scalar[8] = (unsigned long long)n_runs + n_tail;  // list length
            h_scalar[9] = n_runs;                               // work cursor: behind the runs that are done
            HIP_TRY(hipMemcpyAsync(d_split, h_scalar + 8, 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_split + 24, h_scalar + 9, 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(d_split + kOffMeta + (size_t)n_runs * 64, 0, (size_t)n_tail * 64, s));
            RC_TRY(launch_runs(n_tail));
            HIP_TRY(hipMemcpyAsync(h_split + kOffMeta + (size_t)n_runs * 64, d_split + kOffMeta + (size_t)n_runs * 64, (size_t)n_tail * 64,
                                   hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, kCtrBytes, hipMemcpyDeviceToHost, s));
            RC_TRY(wd_sync(idx, cx, s, "the rest of the cut segments"));
            h_scalar[8] = n_runs;  // (a second attempt of the call -- record buffer too small -- starts from the planned list)
            HIP_TRY(hipMemcpyAsync(d_split, h_scalar + 8, 8, hipMemcpyHostToDevice, s));
            for (const Tail &t : tails) {
                const bool gave_up = h_meta[(size_t)t.run * 16 + 4] != 0u;
                if (settle_tail(t.f, held_base.data() + t.held_at, t.base, gave_up, h_fix + t.run_base, h_fix + t.run) == JoinAction::whole_again) {
                    h_again[n_again++] = t.g_seg0;
                    remember(t.g_seg0, 0u, 0u, 0u);  // (more arms than the long shape holds: not a matter of the warm-up)
                }
            }
            RC_TRY(apply_fix());
        }
        if (n_again) {
            HIP_TRY(hipMemcpyAsync(d_split + kOffAgain, h_again, (size_t)n_again * 4, hipMemcpyHostToDevice, s));
            // (what the whole segment overflows goes the way of tier 3's own.  cap_limit is the option's, as in the tail
            // runs above and in tier 3's own launch -- whether or not an early re-run came before)
            RC_TRY(rerun_list(Tiers::kRunsTier, reinterpret_cast<const uint32_t *>(d_split + kOffAgain), n_again, Tiers::kRunsTier, test_cap()));
        }
        HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, kCtrBytes, hipMemcpyDeviceToHost, s));
        RC_TRY(wd_sync(idx, cx, s, "the ranges of the cut segments"));
    }
    return 0;
}

}  // namespace asgart
