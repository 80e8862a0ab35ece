// call_stats.hpp -- the entry points that read, or launch kernels over, what the last search call left in its context:
// asgart_get_stats, asgart_fill_counts, asgart_fill_tally, asgart_tier_segments.
// Part of pipeline.hip, the one translation unit that launches the search kernels.
#pragma once
#include "search_call.hpp"

using namespace asgart;

// f(SlotT{}) for the slot width of the index: 64-bit positions (idx->wide) or 32-bit
template <class F>
static void by_slot(const asgart_index *idx, F f) {
    if (idx->wide) f(uint64_t{});
    else f(uint32_t{});
}

extern "C" {

int32_t asgart_tier_segments(asgart_index *idx, uint64_t *out) {
    if (!idx || !out) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    idx->acquire_all();
    const SearchCtx &cx = idx->ctx[idx->last_ctx];
    for (int i = 0; i < 8; ++i) out[i] = cx.has_last ? cx.tier_segments[i] : 0;
    idx->release_all();
    return 0;
}

// the 18 sums of fill_account_kernel over what the last search call left in its context's workspace
static int32_t fill_account(asgart_index *idx, unsigned long long *acct) {
    for (int j = 0; j < kFillAcct; ++j) acct[j] = 0;
    idx->acquire_all();
    SearchCtx &cx = idx->ctx[idx->last_ctx];
    int32_t rc = [&]() -> int32_t {
        if (!cx.has_last || !cx.last_P) return 0;
        REFUSE_POISONED(idx);
        HIP_TRY(hipSetDevice(idx->device));
        unsigned long long *d_ctr = cx.ws.counters.as<unsigned long long>();
        hipStream_t s = cx.stream;
        const RunParams &rp = cx.last_rp;
        HIP_TRY(hipMemsetAsync(d_ctr + CT_FILL_ACCT, 0, kFillAcct * 8, s));
        const unsigned grid = std::min<uint32_t>(rp.n_tiles(1024u), 1024u);
        const uint32_t *big_list = cx.ws.big_list.as<uint32_t>();
        const uint32_t *ranked_top = big_list + (rp.g_hi - rp.g_lo);
        fill_account_kernel<<<grid, 256, 0, s>>>(rp, cx.ws.p_raw.as<uint32_t>() - rp.g_lo, cx.ws.p_filt.as<uint32_t>() - rp.g_lo,
                                                 big_list, ranked_top, d_ctr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(read_back(acct, d_ctr + CT_FILL_ACCT, kFillAcct * 8, s));  // (polled drain first: common.hpp)
        return 0;
    }();
    idx->release_all();
    return rc;
}

int32_t asgart_fill_counts(asgart_index *idx, uint64_t *out) {
    if (!idx || !out) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    unsigned long long acct[kFillAcct];
    RC_TRY(fill_account(idx, acct));
    for (int j = 0; j < 6; ++j) out[j] = acct[j];
    return 0;
}

int32_t asgart_fill_tally(asgart_index *idx, uint64_t *out) {
    if (!idx || !out) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    unsigned long long acct[kFillAcct];
    RC_TRY(fill_account(idx, acct));
    for (int j = 0; j < 12; ++j) out[j] = acct[6 + j];
    return 0;
}

int32_t asgart_lookup_account(asgart_index *idx, uint64_t *out) {
    if (!idx || !out) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    idx->acquire_all();
    for (int j = 0; j < (int)LA_COUNT; ++j) out[j] = idx->lookup_acct[j];
    idx->release_all();
    return 0;
}

int32_t asgart_run_dir_info(asgart_index *idx, uint64_t *out) {
    if (!idx || !out) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    idx->acquire_all();
    const bool have = idx->d_rdir != nullptr;
    out[0] = have ? idx->rdir_buckets * kRunDirBucketBytes : 0;
    out[1] = have ? idx->rdir_buckets : 0;
    out[2] = have ? idx->rdir_T : 0;
    out[3] = have ? idx->rdir_inserted : 0;
    out[4] = idx->rdir_full;  // (also of a directory the index went without: every run it would have held)
    out[5] = idx->rdir_hits;
    out[6] = idx->rdir_misses;
    out[7] = (uint64_t)idx->run_dir_env.on;
    idx->release_all();
    return 0;
}

int32_t asgart_get_stats(asgart_index *idx, uint32_t flags, asgart_stats *out) {
    if (!idx || !out) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    idx->acquire_all();
    // bits 8.. of flags select a specific context (ASGART_STATS_CTX(i) = (i+1) << 8); default:
    // the context of the most recent search call
    const int sel = (int)((flags >> 8) & 0xFFu);
    SearchCtx &cx = idx->ctx[sel >= 1 && sel <= kNumCtx ? sel - 1 : idx->last_ctx];
    int32_t rc = [&]() -> int32_t {
        if ((flags & (ASGART_STATS_YARDSTICK | ASGART_STATS_RAW_HITS)) && cx.has_last && cx.last_P && !cx.raw_done) {
            // raw_hits of the last call: summed up now, from the per-probe arrays it left in this context's workspace (a probe
            // the position filter answered has no interval there: it is looked up now)
            REFUSE_POISONED(idx);
            HIP_TRY(hipSetDevice(idx->device));
            unsigned long long *d_ctr = cx.ws.counters.as<unsigned long long>();
            hipStream_t s = cx.stream;
            const RunParams &rp = cx.last_rp;
            HIP_TRY(hipMemsetAsync(d_ctr + CT_RAW_HITS, 0, 8, s));
            const unsigned g_raw = std::min<uint32_t>(rp.n_tiles(1024u), 256u * 16u);
            by_slot(idx, [&](auto slot_tag) {
                using SlotT = decltype(slot_tag);
                raw_hits_kernel<SlotT><<<g_raw, 256, 0, s>>>(idx->view<SlotT>(), rp, cx.ws.p_filt.as<uint32_t>() - rp.g_lo,
                                                             cx.ws.p_raw.as<uint32_t>() - rp.g_lo, d_ctr + CT_RAW_HITS);
            });
            HIP_TRY(hipGetLastError());
            unsigned long long v = 0;
            HIP_TRY(read_back(&v, d_ctr + CT_RAW_HITS, 8, s));  // (polled drain first: common.hpp)
            cx.stats.raw_hits = v;
            cx.raw_done = true;
        }
        if ((flags & ASGART_STATS_YARDSTICK) && cx.has_last && cx.last_P) {
            REFUSE_POISONED(idx);
            HIP_TRY(hipSetDevice(idx->device));
            unsigned long long *d_ctr = cx.ws.counters.as<unsigned long long>();
            hipStream_t s = cx.stream;
            HIP_TRY(hipMemsetAsync(d_ctr + CT_BISECT, 0, 8, s));
            RunParams rp = cx.last_rp;
            for (uint32_t p = 0; p < rp.n_passes && p < 4u; ++p) {  // (the position bits as they are now)
                rp.pbits[p] = idx->opt.posbits ? idx->d_pbits[rp.mode_of_pass(p)] : nullptr;
                // (a pass whose position bits were blank when the call ran looked every probe up)
                if ((rp.blank >> p) & 1u) rp.pbits[p] = nullptr;
            }
            const unsigned g = rp.n_tiles(256u);
            by_slot(idx, [&](auto slot_tag) {
                using SlotT = decltype(slot_tag);
                yardstick_kernel<SlotT><<<g, 256, 0, s>>>(idx->view<SlotT>(), rp, cx.ws.p_filt.as<uint32_t>() - rp.g_lo, d_ctr);
            });
            HIP_TRY(hipGetLastError());
            // accounting pass of the probe-search kernels (same control flow, loads and stores priced
            // in bytes instead of executed); the work list of the large intervals is the one the
            // call left in the workspace
            HIP_TRY(hipMemsetAsync(d_ctr + CT_ALG_BYTES, 0, 16, s));
            HIP_TRY(hipMemsetAsync(d_ctr + CT_ALG_BYTES16, 0, 8, s));
            HIP_TRY(hipMemsetAsync(d_ctr + CT_LOOKUP_ACCT, 0, (size_t)LA_COUNT * 8, s));
            const unsigned gp = rp.n_tiles((uint32_t)kProbeBlock);
            by_slot(idx, [&](auto slot_tag) {
                using SlotT = decltype(slot_tag);
                IndexView<SlotT> ix = idx->view<SlotT>();
                probe_count_kernel<SlotT, true><<<gp, kProbeThreads, 0, s>>>(
                    ix, rp, nullptr, nullptr, nullptr, nullptr, nullptr, d_ctr);
                big_count_kernel<SlotT, true><<<2048, 256, 0, s>>>(
                    ix, rp, cx.ws.p_lo.as<SlotT>() - rp.g_lo, cx.ws.p_raw.as<uint32_t>() - rp.g_lo, nullptr,
                    cx.ws.big_list.as<uint32_t>(), d_ctr);
                if (ix.sap)
                    rank_count_kernel<SlotT, true><<<2048, 256, 0, s>>>(
                        ix, rp, cx.ws.p_lo.as<SlotT>() - rp.g_lo, cx.ws.p_raw.as<uint32_t>() - rp.g_lo, nullptr,
                        cx.ws.rank_list.as<uint32_t>(), nullptr, nullptr, 0, d_ctr);  // (no list is written: the bytes do not depend on the ranked fill)
            });
            HIP_TRY(hipGetLastError());
            unsigned long long v = 0, ab[2] = {0, 0}, a16 = 0;
            HIP_TRY(read_back(&v, d_ctr + CT_BISECT, 8, s));  // (polled drain first: common.hpp)
            HIP_TRY(read_back(ab, d_ctr + CT_ALG_BYTES, 16, s));
            HIP_TRY(read_back(&a16, d_ctr + CT_ALG_BYTES16, 8, s));
            unsigned long long la[LA_COUNT];
            HIP_TRY(read_back(la, d_ctr + CT_LOOKUP_ACCT, sizeof(la), s));
            for (int j = 0; j < (int)LA_COUNT; ++j) idx->lookup_acct[j] = la[j];
            idx->rdir_hits = la[LA_DIR_HIT];
            idx->rdir_misses = la[LA_DIR_MISS];
            cx.stats.bisect_steps = v;
            cx.stats.search_bytes = ab[0];
            cx.stats.probes_filter_rejected = ab[1];
            cx.stats.search_bytes_wide_loads = a16;
        }
        *out = cx.stats;
        return 0;
    }();
    idx->release_all();
    return rc;
}

}  // extern "C"
