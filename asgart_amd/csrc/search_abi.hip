// search_abi.hip -- the C ABI of a search: asgart_search_duplications and its sharded and multi-device forms, the result
// object's accessors, asgart_probe_hits, and the host rules that tests read through the ABI.  Host only: nothing is
// launched from here, the calls go through run_search (pipeline.hip).
#include "device_base.hpp"

#include <algorithm>
#include <string>
#include <thread>

using namespace asgart;

extern "C" {

static int32_t search_shard_impl(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                 const asgart_settings *settings, int32_t shard, int32_t n_shards,
                                 volatile uint64_t *progress, asgart_families **out) {
    if (!out) {
        set_error("out is NULL");
        return ASGART_E_ARG;
    }
    *out = nullptr;
    std::unique_ptr<asgart_families> f = new_families();
    if (!f) return ASGART_E_OOM;
    RC_TRY(run_search(idx, chunks, n_chunks, settings, shard, n_shards, false, f.get(), nullptr, nullptr, nullptr, progress));
    *out = f.release();
    return 0;
}

int32_t asgart_search_duplications_shard(asgart_index *idx, const uint64_t *chunks,
                                         int64_t n_chunks, const asgart_settings *settings,
                                         int32_t shard, int32_t n_shards, asgart_families **out) {
    return search_shard_impl(idx, chunks, n_chunks, settings, shard, n_shards, nullptr, out);
}

int32_t asgart_search_duplications_ex(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                      const asgart_settings *settings, int32_t shard, int32_t n_shards,
                                      volatile uint64_t *progress, asgart_families **out) {
    return search_shard_impl(idx, chunks, n_chunks, settings, shard, n_shards, progress, out);
}

int32_t asgart_search_duplications(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                   const asgart_settings *settings, volatile uint64_t *progress,
                                   asgart_families **out) {
    int32_t rc = search_shard_impl(idx, chunks, n_chunks, settings, 0, 1, progress, out);
    // (also written earlier, when the chip-wide phases were over: run_tiers, call_tiers.hpp)
    if (rc == 0 && progress) fill_progress(progress, chunks + 1, 2, n_chunks, *settings);
    return rc;
}

int32_t asgart_search_duplications_multi(asgart_index *const *indices, int32_t n_devices,
                                         const uint64_t *chunks, int64_t n_chunks,
                                         const asgart_settings *settings, volatile uint64_t *progress,
                                         asgart_families **out) {
    if (!out) {
        set_error("out is NULL");
        return ASGART_E_ARG;
    }
    *out = nullptr;
    if (!indices || n_devices < 1 || n_devices > 64) {
        set_error("bad argument: %d devices", n_devices);
        return ASGART_E_ARG;
    }
    for (int32_t r = 0; r < n_devices; ++r)
        if (!indices[r] || indices[r]->n != indices[0]->n || indices[r]->n_sa != indices[0]->n_sa) {
            set_error("index %d is NULL or not a replica of index 0", r);
            return ASGART_E_ARG;
        }
    // one host thread per device; shard r of n_devices (no exchange between shards)
    std::vector<asgart_families> parts((size_t)n_devices);
    std::vector<int32_t> rcs((size_t)n_devices, 0);
    std::vector<std::string> errs((size_t)n_devices);
    std::vector<std::thread> workers;
    for (int32_t r = 0; r < n_devices; ++r)
        workers.emplace_back([&, r]() {
            rcs[r] = run_search(indices[r], chunks, n_chunks, settings, r, n_devices, false, &parts[r], nullptr,
                                nullptr, nullptr, nullptr);
            if (rcs[r] != 0) errs[r] = asgart_last_error();  // the message is thread-local
        });
    for (auto &t : workers) t.join();
    for (int32_t r = 0; r < n_devices; ++r)
        if (rcs[r] != 0) {
            set_error("shard %d of %d: %s", r, n_devices, errs[r].c_str());
            return rcs[r];
        }
    std::unique_ptr<asgart_families> f = new_families();
    if (!f) return ASGART_E_OOM;
    // merge the shards' families by key (segment start probe, family ordinal): reference order, whichever way
    // the segments were dealt out
    struct Ref {
        uint64_t key;
        int32_t r;
        uint32_t j;
    };
    std::vector<Ref> refs;
    for (int32_t r = 0; r < n_devices; ++r)
        for (size_t j = 0; j < parts[r].fam_keys.size(); ++j) refs.push_back(Ref{parts[r].fam_keys[j], r, (uint32_t)j});
    std::stable_sort(refs.begin(), refs.end(), [](const Ref &a, const Ref &b) { return a.key < b.key; });
    f->fam_offsets.assign(1, 0);
    for (const Ref &e : refs) {
        const asgart_families &p = parts[e.r];
        f->sds.insert(f->sds.end(), p.sds.begin() + (ptrdiff_t)p.fam_offsets[e.j], p.sds.begin() + (ptrdiff_t)p.fam_offsets[e.j + 1]);
        f->fam_offsets.push_back(f->sds.size());
        f->fam_keys.push_back(e.key);
    }
    if (progress && settings) fill_progress(progress, chunks + 1, 2, n_chunks, *settings);
    *out = f.release();
    return 0;
}

void asgart_families_counts(const asgart_families *f, uint64_t *n_families, uint64_t *n_sds) {
    if (n_families) *n_families = f ? f->fam_offsets.size() - 1 : 0;
    if (n_sds) *n_sds = f ? f->sds.size() : 0;
}

void asgart_families_copy(const asgart_families *f, uint64_t *fam_offsets, asgart_proto_sd *sds) {
    if (!f) return;
    if (fam_offsets) memcpy(fam_offsets, f->fam_offsets.data(), f->fam_offsets.size() * 8);
    if (sds && !f->sds.empty()) memcpy(sds, f->sds.data(), f->sds.size() * sizeof(asgart_proto_sd));
}

void asgart_families_keys(const asgart_families *f, uint64_t *keys) {
    if (f && keys && !f->fam_keys.empty()) memcpy(keys, f->fam_keys.data(), f->fam_keys.size() * 8);
}

void asgart_families_free(asgart_families *f) { delete f; }

int64_t asgart_probe_hits(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                          const asgart_settings *settings, uint8_t *status, uint64_t *row_offsets,
                          uint64_t *hits, uint64_t *n_hits) {
    std::vector<uint8_t> st;
    std::vector<uint64_t> ro, hv;
    int32_t rc = run_search(idx, chunks, n_chunks, settings, 0, 1, true, nullptr, &st, &ro, &hv, nullptr);
    if (rc != 0) return rc;
    if (n_hits) *n_hits = hv.size();
    if (status) {
        if (!st.empty()) memcpy(status, st.data(), st.size());
        memcpy(row_offsets, ro.data(), ro.size() * 8);
        if (!hv.empty()) memcpy(hits, hv.data(), hv.size() * 8);
    }
    return (int64_t)st.size();
}

// ---- host rules, as the search applies them ----------------------------------------------------------------------------------
int32_t asgart_ranked_fill_takes(uint64_t interval, uint64_t kept, int32_t mode) {
    return ranked_fill_takes(interval, kept, (int)mode) ? 1 : 0;
}

void asgart_hit_rule(uint64_t i, uint64_t s, uint64_t L, int32_t reverse, uint64_t *out) {
    const HitRule hr = hit_rule(i, s, L, reverse != 0);
    out[0] = hr.thr;
    out[1] = hr.self;
}

void asgart_run_dir_rule(uint64_t key, uint64_t lo, uint64_t len, uint64_t n_buckets, uint64_t *out) {
    const uint64_t w = run_dir_pack(lo, len);
    out[0] = w;
    out[1] = run_dir_lo(w);
    out[2] = run_dir_len(w);
    out[3] = run_dir_bucket(key, (uint32_t)std::min<uint64_t>(n_buckets, kRunDirMaxBuckets));
    out[4] = kRunDirEmpty;
}

int32_t asgart_join_cuts(int32_t n_ranges, const uint32_t *cut_held, const uint32_t *flushes, int32_t last_gave_up,
                         int32_t tail_gave_up, uint32_t *fix, uint32_t *settled, uint32_t *out) {
    if (n_ranges < 1 || n_ranges > 4096 || (n_ranges > 1 && !cut_held) || !flushes || !fix || !settled || !out) {
        set_error("asgart_join_cuts: bad argument");
        return ASGART_E_ARG;
    }
    const uint32_t R = (uint32_t)n_ranges;
    std::vector<uint32_t> held(R);
    const JoinVerdict jv = join_segment(R, cut_held, flushes, 1, last_gave_up != 0, fix, held.data());
    JoinAction after = jv.action;
    std::copy(fix, fix + R, settled);
    settled[R] = kFixDropped;  // (no tail run)
    if (jv.action == JoinAction::tail_run) after = settle_tail(jv.f, held.data(), jv.tail_base, tail_gave_up != 0, settled, settled + R);
    out[0] = jv.f;
    out[1] = (uint32_t)jv.action;
    out[2] = jv.tail_base;
    out[3] = (uint32_t)after;
    return 0;
}

uint32_t asgart_split_warm_next(uint32_t warm_used, uint32_t need, uint32_t range_len, uint64_t split_warm_max) {
    return split_warm_next(warm_used, need, range_len, split_warm_max);
}

}  // extern "C"
