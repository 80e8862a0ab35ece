// pipeline.hip -- host driver of the probe -> search -> extend pipeline: the one translation unit that launches the
// search kernels (place_dev.hpp and others define non-template kernels: a second such unit would define them again).
// The state of a call and the list of its stages: search_call.hpp; a header per stage group, in the order run() takes
// them; the entry points that launch for the statistics: call_stats.hpp.  The host-only entry points of a search live in
// search_abi.hip and passes.hip, the tier plan in tiers.hip.
//
// Replaces the body of SearchDuplications::run, reference
// src/bin/asgart.rs:201-253 (chunk fan-out, needle preparation, automaton,
// left fix-up, fold in chunk order).
#include "search_call.hpp"
#include "call_setup.hpp"
#include "call_front.hpp"
#include "call_place.hpp"
#include "call_tiers.hpp"
#include "call_join.hpp"
#include "call_records.hpp"

namespace asgart {

template <class SlotT>
int32_t SearchCall<SlotT>::run() {
    RC_TRY(setup());
    if (nothing_to_do) return 0;
    for (int win_try = 0;; ++win_try) {  // (a sharded call widens its halos until every decision is safe)
        if (win_try > 40) {
            set_error("internal: shard window did not converge");
            return ASGART_E_CAP;
        }
        set_window();
        bool ambiguous = false;
        RC_TRY(front(&ambiguous));
        if (ambiguous) {
            look_back *= 8;
            continue;
        }
        // (the hit rows are being filled on a stream of their own; place() waits for them where it needs them)
        if (want_csr || !(fam_out && n_seg)) HIP_TRY(hipStreamWaitEvent(s, cx.ev[EV_HIT_ROWS], 0));
        if (want_csr) RC_TRY(csr_out());
        if (fam_out && n_seg) {
            RC_TRY(place());
            for (int attempt = 0;; ++attempt) {  // (again with a larger record buffer when it overflowed)
                RC_TRY(run_tiers(attempt));
                RC_TRY(join_ranges());
                RC_TRY(finish_tiers());
                if (h_ctr[CT_RANOUT]) break;
                if (h_ctr[CT_SD] <= rec_cap) break;
                if (attempt >= 3) {
                    set_error("internal: record buffer keeps overflowing");
                    return ASGART_E_CAP;
                }
                rec_cap = h_ctr[CT_SD] * 2;
            }
            if (h_ctr[CT_RANOUT]) {  // a segment runs past the look-ahead halo: widen it
                look_ahead *= 8;
                continue;
            }
            RC_TRY(records());
        } else {
            HIP_TRY(hipEventRecord(cx.ev[EV_EXTENDED], s));
            RC_TRY(wd_sync(idx, cx, s, "the hit rows"));
        }
        break;
    }
    return fill_stats();
}

template <class SlotT>
static int32_t run_search_t(asgart_index *idx, SearchCtx &cx, const uint64_t *chunks, int64_t n_chunks_pass,
                            const asgart_settings *sts, int32_t n_passes, int32_t shard, int32_t n_shards,
                            bool want_csr, asgart_families *const *fams,
                            std::vector<uint8_t> *status_out, std::vector<uint64_t> *rowoff_out,
                            std::vector<uint64_t> *hits_out) {
    // (on the heap: the call's state holds its kernels' parameter blocks and a few KB of tables)
    std::unique_ptr<SearchCall<SlotT>> call(new (std::nothrow) SearchCall<SlotT>(idx, cx, chunks, n_chunks_pass, sts, n_passes, shard,
                                                                                n_shards, want_csr, fams, status_out, rowoff_out, hits_out));
    if (!call) {
        set_error("out of host memory");
        return ASGART_E_OOM;
    }
    return call->run();
}


// n_passes > 1: ONE job over the probes of all passes (sts differ in reverse / complement only; checked by the caller);
// fams: n_passes result objects, or null (the CSR surface of a single pass).
int32_t run_search_passes(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                          const asgart_settings *sts, int32_t n_passes, int32_t shard, int32_t n_shards, bool want_csr,
                          asgart_families *const *fams, std::vector<uint8_t> *status_out,
                          std::vector<uint64_t> *rowoff_out, std::vector<uint64_t> *hits_out,
                          volatile uint64_t *progress) {
    if (!idx || !sts || n_passes < 1 || n_passes > 4 || n_chunks < 0 || (n_chunks && !chunks)) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    const asgart_settings *const st = &sts[0];
    if (st->max_gap_size == 0) {
        // the CLI always passes gap + probe_size (reference src/bin/asgart.rs:681), never 0
        set_error("max_gap_size must be >= 1 (it includes probe_size, src/bin/asgart.rs:681)");
        return ASGART_E_ARG;
    }
    if (n_shards < 1 || shard < 0 || shard >= n_shards || (n_passes > 1 && (want_csr || progress))) {
        set_error("bad shard %d of %d", shard, n_shards);
        return ASGART_E_ARG;
    }
    REFUSE_POISONED(idx);
    HIP_TRY(hipSetDevice(idx->device));
    // take a free per-call context; the keys can only change while no context is in use
    int which = 0;
    for (;;) {
        SearchCtx &probe = idx->acquire_one(&which);
        (void)probe;
        // An orientation's position bits start blank and its searches fill them in.  The position-sorted lists cost more
        // than they save in ONE pass (option lazy_aux): the index gets them at its second call.
        bool want_sap, ready;
        int need_blank = -1;  // an orientation of this call whose blank position bits are due and missing
        {
            std::lock_guard<std::mutex> lk(idx->mu);
            ready = idx->k == st->probe_size;
            const bool filterable = !(idx->opt.posbits == 0 || idx->trimmed || st->probe_size > (uint64_t)kMaxKey);
            for (int32_t p = 0; p < n_passes && need_blank < 0; ++p) {
                const uint32_t mode = mode_of_settings(sts[p]);
                if (filterable && ready && !idx->filter_off[mode] && !idx->d_pbits[mode]) need_blank = mode;
            }
            want_sap = !(idx->opt.lazy_aux && (!ready || idx->calls_total == 0)) && !idx->sap_tried;
            if (ready && need_blank < 0 && !(want_sap && !idx->d_sap)) break;
        }
        idx->release_one(which);
        if (!ready) RC_TRY(index_prepare(idx, st->probe_size));
        else if (want_sap && !idx->d_sap) RC_TRY(index_prepare_sap(idx, st->probe_size));
        else RC_TRY(index_prepare_learned_bits(idx, st->probe_size, need_blank));
    }
    SearchCtx &cx = idx->ctx[which];
    cx.progress = progress;
    int32_t rc;
    if (idx->wide)
        rc = run_search_t<uint64_t>(idx, cx, chunks, n_chunks, sts, n_passes, shard, n_shards, want_csr, fams,
                                    status_out, rowoff_out, hits_out);
    else
        rc = run_search_t<uint32_t>(idx, cx, chunks, n_chunks, sts, n_passes, shard, n_shards, want_csr, fams,
                                    status_out, rowoff_out, hits_out);
    cx.progress = nullptr;
    bool trim_now = false;
    {   // (counted in PASSES: a host that runs the direct and the -RC pass as one passes call -- the CLI's shape -- has made its
        // two searches when that call returns, and must not sit on the sorter's ~100 GB of scratch until it destroys the index)
        std::lock_guard<std::mutex> lk(idx->mu);
        const uint64_t before = idx->calls_total;
        idx->calls_total += (uint64_t)n_passes;
        for (int32_t p = 0; p < n_passes; ++p) ++idx->pbits_uses[mode_of_settings(sts[p])];
        trim_now = idx->opt.cache_calls > 0 && before < (uint64_t)idx->opt.cache_calls && idx->calls_total >= (uint64_t)idx->opt.cache_calls;
    }
    if (trim_now) {  // (option cache_calls: what the index build released goes back to the device now -- behind the caller's back:
                     // the hipFree of ~100 GB is not this call's business)
        const int dev = idx->device;
        background_call([dev]() {
            if (hipSetDevice(dev) == hipSuccess) BlockCache::trim();
            (void)hipGetLastError();
        });
    }
    if (rc == 0 && fams && n_shards == 1 && n_passes == 1) {
        // what asgart_search_duplications_passes orders by when it pipelines single-pass calls: the shortest extension seen
        // for the orientation (a call that shared the chip with another one measures longer, and the order must not flip
        // because of that)
        std::lock_guard<std::mutex> lk(idx->mu);
        double &t = idx->tail_ms[mode_of_settings(*st)];
        t = t < 0.0 ? cx.stats.ms_extend : std::min(t, cx.stats.ms_extend);
    }
    idx->release_one(which);
    return rc;
}

int32_t run_search(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                   const asgart_settings *st, int32_t shard, int32_t n_shards, bool want_csr,
                   asgart_families *fam_out, std::vector<uint8_t> *status_out,
                   std::vector<uint64_t> *rowoff_out, std::vector<uint64_t> *hits_out,
                   volatile uint64_t *progress) {
    asgart_families *one[1] = {fam_out};
    return run_search_passes(idx, chunks, n_chunks, st, 1, shard, n_shards, want_csr, fam_out ? one : nullptr, status_out,
                             rowoff_out, hits_out, progress);
}

}  // namespace asgart

#include "call_stats.hpp"
