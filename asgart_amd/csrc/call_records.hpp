// call_records.hpp -- stages records and fill_stats of a search call.
// Part of pipeline.hip, the one translation unit that launches the search kernels (search_call.hpp has the stage list).
#pragma once
#include "search_call.hpp"

namespace asgart {

// ---- records -> reference order -> families per pass ----------------------------------------------------------------------
template <class SlotT>
int32_t SearchCall<SlotT>::records() {
    HIP_TRY(hipEventRecord(cx.ev[EV_EXTENDED], s));
    const uint64_t n_rec = h_ctr[CT_SD];
    if (n_rec) {
        void *hp = nullptr;
        RC_TRY(cx.pinned((size_t)n_rec * sizeof(SdRec), &hp));
        h_recs = static_cast<const SdRec *>(hp);
        n_hrec = (size_t)n_rec;
    }
    // Reference order: chunk order, discovery order inside the chunk, arm order
    // inside the family == (segment start probe, family ordinal, creation number): sorted on
    // the GPU.  A tombstone voids its family; segments re-run by a later tier emit some
    // records twice (same key): keep one copy.
    if (n_rec) {
        RC_TRY(sort_records(w, w.fam_sds.as<SdRec>(), n_rec, s));
        HIP_TRY(hipMemcpyAsync(const_cast<SdRec *>(h_recs), w.rec_sorted.p, (size_t)n_rec * sizeof(SdRec),
                               hipMemcpyDeviceToHost, s));
    }
    const auto t_post0 = std::chrono::steady_clock::now();
    RC_TRY(wd_sync(idx, cx, s, "the ordering of the records"));
    const auto t_post1 = std::chrono::steady_clock::now();
    // (sorted by segment start probe: pass 0's families first, then pass 1's ...; a family's key counts probes from
    // the start of its OWN pass, so that it equals the key a single-pass call gives the same family)
    // Assembly: the records are read once (48 bytes each: a memory-bound loop) -- large lists by up to four host threads,
    // each over a slice that starts at a family boundary, their parts joined in order.
    using Part = SearchCtx::FamPart;  // (kept by the call context: fresh vectors of this size cost their page faults every call)
    auto assemble = [&](size_t b0, size_t b1, Part &out) {
        int32_t pass = 0;
        for (size_t f0 = b0; f0 < b1;) {
            if (h_recs[f0].g_start == kVoidStart) break;  // unused slots of the waves' record chunks: sorted last
            size_t f1 = f0;
            while (f1 < n_hrec && h_recs[f1].g_start == h_recs[f0].g_start && h_recs[f1].fam_seq == h_recs[f0].fam_seq) ++f1;
            while (pass + 1 < n_passes && h_recs[f0].g_start >= (uint32_t)(pass + 1) * K) ++pass;
            if (h_recs[f1 - 1].create_seq != kTombstone) {
                std::vector<asgart_proto_sd> &sds = out.sds[pass];
                for (size_t j = f0; j < f1; ++j) {
                    if (j > f0 && h_recs[j].create_seq == h_recs[j - 1].create_seq) continue;
                    sds.push_back(h_recs[j].sd);
                }
                out.ends[pass].push_back(sds.size());
                out.keys[pass].push_back(((uint64_t)(lo_lim + (h_recs[f0].g_start - (uint32_t)pass * K)) << 32) |
                                         (uint64_t)h_recs[f0].fam_seq);
            }
            f0 = f1;
        }
    };
    const size_t n_parts = n_hrec >= (1u << 17) ? 4 : 1;
    size_t bound[5] = {0, 0, 0, 0, n_hrec};
    for (size_t t = 1; t < n_parts; ++t) {  // slice boundaries moved forward to the next family start
        size_t b = std::max(bound[t - 1], n_hrec * t / n_parts);
        while (b > 0 && b < n_hrec && h_recs[b].g_start == h_recs[b - 1].g_start && h_recs[b].fam_seq == h_recs[b - 1].fam_seq) ++b;
        bound[t] = b;
    }
    for (size_t t = n_parts; t < 4; ++t) bound[t] = n_hrec;
    std::vector<Part> &parts = cx.fam_parts;
    parts.resize(4);
    for (size_t t = 0; t < 4; ++t)
        for (int32_t p = 0; p < 4; ++p) {
            parts[t].sds[p].clear();
            parts[t].ends[p].clear();
            parts[t].keys[p].clear();
            if (t < n_parts && p < n_passes)
                parts[t].sds[p].reserve((bound[t + 1] - bound[t]) / (size_t)n_passes + (bound[t + 1] - bound[t]) / 4 + 16);
        }
    {
        std::vector<std::thread> workers;
        for (size_t t = 1; t < n_parts; ++t) workers.emplace_back([&, t]() { assemble(bound[t], bound[t + 1], parts[t]); });
        assemble(bound[0], bound[1], parts[0]);
        for (auto &th : workers) th.join();
    }
    for (int32_t p = 0; p < n_passes; ++p) {
        asgart_families *const fo = fams[p];
        size_t tot = 0, nf = 0;
        for (const Part &pt : parts) {
            tot += pt.sds[p].size();
            nf += pt.ends[p].size();
        }
        if (!tot && !nf) continue;
        fo->sds.reserve(fo->sds.size() + tot);
        fo->fam_offsets.reserve(fo->fam_offsets.size() + nf);
        fo->fam_keys.reserve(fo->fam_keys.size() + nf);
        for (const Part &pt : parts) {
            const size_t at = fo->sds.size();
            fo->sds.insert(fo->sds.end(), pt.sds[p].begin(), pt.sds[p].end());
            for (uint64_t e : pt.ends[p]) fo->fam_offsets.push_back(at + e);
            fo->fam_keys.insert(fo->fam_keys.end(), pt.keys[p].begin(), pt.keys[p].end());
        }
    }
    if (opt.debug)
        fprintf(stderr, "[asgart] records: %llu slots; ordering + copy to the host %.1f ms, families assembled in %.1f ms\n",
                (unsigned long long)n_rec, std::chrono::duration<double, std::milli>(t_post1 - t_post0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_post1).count());
    return 0;
}

template <class SlotT>
int32_t SearchCall<SlotT>::fill_stats() {
    // ---- stats ------------------------------------------------------------------
    asgart_stats &stt = cx.stats;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, cx.ev[EV_SEARCH], cx.ev[EV_SEARCHED]));
    stt.ms_search = ms;
    HIP_TRY(hipEventElapsedTime(&ms, cx.ev[EV_SEARCHED], cx.ev[EV_SCANNED]));
    stt.ms_scan = ms;
    HIP_TRY(hipEventElapsedTime(&ms, cx.ev[EV_FILL], cx.ev[EV_HIT_ROWS]));
    stt.ms_fill = ms;
    HIP_TRY(hipEventElapsedTime(&ms, cx.ev[EV_HIT_ROWS], cx.ev[EV_EXTENDED]));
    stt.ms_extend = ms;
    stt.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() -
                                                            t_host0).count();
    stt.probes_n_skipped = h_ctr[CT_N_SKIPPED];
    stt.probes_searched = h_ctr[CT_SEARCHED];
    stt.probes_card_skipped = h_ctr[CT_CARD_SKIPPED];
    stt.probes_with_hits = h_ctr[CT_WITH_HITS];
    stt.raw_hits = 0;  // (asgart_get_stats sums them up when asked: raw_hits_kernel)
    stt.filtered_hits = total_hits;
    stt.segments = n_seg;
    stt.families = stt.proto_sds = 0;
    for (int32_t p = 0; fam_out && p < n_passes; ++p) {
        stt.families += fams[p]->fam_offsets.size() - 1;
        stt.proto_sds += fams[p]->sds.size();
    }
    stt.passes = (uint64_t)n_passes;
    stt.search_launches = 1;
    stt.overflow_segments = n_overflow;
    stt.heavy_segments = n_heavy;

    stt.ms_extend_tier2 = ms_tier2;
    stt.ms_longest_tier = ms_longest_tier;
    stt.ms_longest_segment = ms_longest_segment;
    stt.split_segments = n_split_segments;
    stt.split_refused = n_split_refused;
    HIP_TRY(hipEventElapsedTime(&ms, cx.ev[EV_SEARCH], cx.ev[EV_PROBE_COUNT]));
    stt.ms_probe_count = ms;
    cx.has_last = true;
    cx.raw_done = false;
    return 0;
}

}  // namespace asgart
