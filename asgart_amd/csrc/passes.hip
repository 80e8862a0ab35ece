// passes.hip -- asgart_search_duplications_passes: the passes (orientations) of one chunk list as ONE job, or as
// pipelined single-pass calls on the two call contexts, and the measured verdict between the two
// (asgart_index::FuseVerdict, index.hpp).  Host only: nothing is launched from here, the calls go through run_search and
// run_search_passes (pipeline.hip).
#include "index.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>

using namespace asgart;

namespace {

// the thread that holds asgart_index::pass_mu says so (index_prepare's prewarm, reached from a call below, must not try
// to lock it again)
struct Owns {
    Owns() { asgart::tl_owns_pass_mu = true; }
    ~Owns() { asgart::tl_owns_pass_mu = false; }
};

// ---- the passes as ONE job (option fuse_passes, default) ------------------------------------------------------------
// Passes that differ in orientation only -- the direct and the -RC run of one genome, what the call exists for --
// share one probe sequence (pass 0's chunks, then pass 1's, ...: chunk order inside each pass as in
// src/bin/asgart.rs:201-253): ONE probe search, scan, hit-row fill and placement over all their probes at full chip
// rate, ONE launch per extension tier over the merged cost-sorted segment list -- every pass's longest segments
// start at t = 0 of the extension on compute units of their own.  A SHARDED call is the same job over the shard's slice
// of every pass (SearchCall::setup: one window per pass).  (Pipelined as two calls on two contexts -- passes_pipelined,
// kept for passes with different settings and for inputs whose extension is ONE segment -- the second pass's front
// crawled behind the first one's persistent extension workgroups: 117 ms instead of 28 at GRCh38 size.)
int32_t passes_as_one_job(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks, const asgart_settings *settings,
                          int32_t n_passes, int32_t shard, int32_t n_shards, asgart_families **out) {
    std::vector<std::unique_ptr<asgart_families>> fams((size_t)n_passes);
    std::vector<asgart_families *> raw;
    for (auto &f : fams) {
        f = new_families();
        if (!f) return ASGART_E_OOM;
        raw.push_back(f.get());
    }
    RC_TRY(run_search_passes(idx, chunks, n_chunks, settings, n_passes, shard, n_shards, false, raw.data(), nullptr, nullptr, nullptr,
                             nullptr));
    for (int32_t j = 0; j < n_passes; ++j) out[j] = fams[(size_t)j].release();
    return 0;
}

// can these passes run as one job?  They differ in orientation only, and together they stay below 2^32 probes.
bool passes_fusable(const asgart_index *idx, const uint64_t *chunks, int64_t n_chunks, const asgart_settings *settings, int32_t n_passes) {
    bool fusable = idx->opt.fuse_passes != 0 && n_passes >= 2 && n_passes <= 4;  // (option fuse_passes)
    for (int32_t j = 1; fusable && j < n_passes; ++j)
        fusable = settings[j].probe_size == settings[0].probe_size && settings[j].max_gap_size == settings[0].max_gap_size &&
                  settings[j].min_duplication_length == settings[0].min_duplication_length &&
                  settings[j].max_cardinality == settings[0].max_cardinality;
    if (fusable) {  // (2^32 probes per call: the passes together)
        const uint64_t k = settings[0].probe_size, step = k / 2;
        uint64_t P1 = 0;
        for (int64_t c = 0; c < n_chunks && step; ++c)
            P1 += probes_in_chunk(chunks[2 * c + 1], k, step, settings[0].min_duplication_length);
        fusable = step && P1 * (uint64_t)n_passes < 0xFFFFFF00ull;
    }
    return fusable;
}

// ---- the passes as pipelined single-pass calls ---------------------------------------------------------------------------
int32_t passes_pipelined(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks, const asgart_settings *settings,
                         int32_t n_passes, int32_t shard, int32_t n_shards, asgart_families **out) {
    // issue order: longest extension first (what is known from earlier calls; an orientation never run yet
    // counts as longest, reversed ones ahead of the others: their tandem arrays are walked against the
    // whole text instead of the part behind the probe)
    std::vector<int32_t> order((size_t)n_passes);
    for (int32_t j = 0; j < n_passes; ++j) order[j] = j;
    double tail_ms[4];
    {   // (a plain call on the other context may be updating them: run_search writes under the same lock)
        std::lock_guard<std::mutex> lk(idx->mu);
        for (int m = 0; m < 4; ++m) tail_ms[m] = idx->tail_ms[m];
    }
    auto weight = [&](int32_t j) {
        const uint32_t mode = mode_of_settings(settings[j]);
        const double t = tail_ms[mode];
        return t >= 0.0 ? t : 1e30 + (settings[j].reverse ? 1e29 : 0.0);
    };
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return weight(a) > weight(b); });
    // one host thread per pass; thread p starts its call when pass p-1 reports its probes as searched
    // (or has returned); a call blocks in the index until one of the two contexts is free
    std::vector<std::unique_ptr<asgart_families>> fams((size_t)n_passes);
    std::vector<int32_t> rcs((size_t)n_passes, 0);
    std::vector<std::string> errs((size_t)n_passes);
    std::vector<std::vector<uint64_t>> prog((size_t)n_passes, std::vector<uint64_t>((size_t)std::max<int64_t>(n_chunks, 1), 0));
    std::vector<std::atomic<int>> finished((size_t)n_passes);
    for (auto &f : finished) f.store(0);
    auto searched = [&](int32_t p) {
        if (finished[p].load(std::memory_order_acquire)) return true;
        const volatile uint64_t *pr = prog[p].data();
        for (int64_t c = 0; c < n_chunks; ++c)
            if (pr[c]) return true;
        return false;
    };
    // the first pass runs on the calling thread, the others on the index's own worker threads
    std::lock_guard<std::mutex> pass_lock(idx->pass_mu);
    Owns owns;
    while ((int32_t)idx->pass_workers.size() + 1 < n_passes) idx->pass_workers.emplace_back(new asgart::PassWorker());
    auto body = [&](int32_t p) {
        if (p > 0)
            while (!searched(p - 1)) std::this_thread::sleep_for(std::chrono::microseconds(100));
        const int32_t j = order[p];
        std::unique_ptr<asgart_families> f = new_families();
        rcs[p] = !f ? ASGART_E_OOM
                    : run_search(idx, chunks, n_chunks, &settings[j], shard, n_shards, false, f.get(), nullptr, nullptr, nullptr,
                                 prog[p].data());
        if (rcs[p] != 0) errs[p] = asgart_last_error();  // the message is thread-local
        else fams[p] = std::move(f);
        finished[p].store(1, std::memory_order_release);
    };
    for (int32_t p = 1; p < n_passes; ++p) idx->pass_workers[(size_t)p - 1]->submit([&body, p]() { body(p); });
    body(0);
    for (int32_t p = 1; p < n_passes; ++p) idx->pass_workers[(size_t)p - 1]->wait();
    for (int32_t p = 0; p < n_passes; ++p)
        if (rcs[p] != 0) {
            set_error("pass %d of %d: %s", order[p], n_passes, errs[p].c_str());
            return rcs[p];
        }
    for (int32_t p = 0; p < n_passes; ++p) out[order[p]] = fams[p].release();
    return 0;
}

// (pipelined: timed for the verdict when it was that verdict's choice -- in a destructor, so that a call that returns
// early stays untimed)
struct TimedPipelined {
    asgart_index *idx;
    bool on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    bool ok = false;
    ~TimedPipelined() {
        if (!on || !ok) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::lock_guard<std::mutex> lk(idx->mu);
        uint64_t refused = 0;
        for (int c = 0; c < asgart::kNumCtx; ++c) refused += idx->ctx[c].stats.split_refused;
        if (!idx->fuse_verdict.note_piped(ms, refused != 0)) return;  // (still learning which ranges join up: not a sample)
        if (idx->opt.debug) fprintf(stderr, "[asgart] passes pipelined, %.1f ms (timed against the passes as one job)\n", ms);
    }
};

}  // namespace

extern "C" {

int32_t asgart_search_duplications_passes(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                          const asgart_settings *settings, int32_t n_passes,
                                          asgart_families **out) {
    return asgart_search_duplications_passes_shard(idx, chunks, n_chunks, settings, n_passes, 0, 1, out);
}

int32_t asgart_search_duplications_passes_shard(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                                const asgart_settings *settings, int32_t n_passes,
                                                int32_t shard, int32_t n_shards, asgart_families **out) {
    if (!out || n_passes < 0 || (n_passes && !settings)) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    for (int32_t j = 0; j < n_passes; ++j) out[j] = nullptr;
    if (!idx || n_chunks < 0 || (n_chunks && !chunks)) {
        set_error("bad argument");
        return ASGART_E_ARG;
    }
    if (n_passes == 0) return 0;
    // ---- decide --------------------------------------------------------------------------------------------------------------
    bool fusable = passes_fusable(idx, chunks, n_chunks, settings, n_passes);
    uint64_t modes_sig = 0;
    for (int32_t j = 0; fusable && j < n_passes; ++j)
        modes_sig = modes_sig * 4u + mode_of_settings(settings[j]);
    // What the calls with these settings have measured decides -- for an unsharded call: what pipelining can win is the
    // other passes' front beside the one long segment, and a shard's front is 1/N of it, while the second pass's front
    // crawling behind the first one's persistent workgroups costs a shard as much as it costs the whole call (GRCh38-
    // shaped, the shards of N = 8 timed alone: 32-64 ms as one job, 47-78 ms pipelined).  Once a call that ran as one
    // job has seen ONE segment be its extension, the calls are timed both ways in turn (one job, pipelined, one job,
    // pipelined) and the faster way is kept.
    const bool may_pipeline = fusable && idx->opt.fuse_passes == 1 && n_shards == 1;
    if (may_pipeline) {
        std::lock_guard<std::mutex> lk(idx->mu);
        const asgart_index::FuseVerdict &v = idx->fuse_verdict;
        if (v.matches(settings, n_passes, modes_sig, shard, n_shards) && v.wants_pipelined()) fusable = false;
    }
    const auto t_call0 = std::chrono::steady_clock::now();
    if (fusable) {
        std::lock_guard<std::mutex> pass_lock(idx->pass_mu);
        Owns owns;
        // ---- run ---------------------------------------------------------------------------------------------------------------
        RC_TRY(passes_as_one_job(idx, chunks, n_chunks, settings, n_passes, shard, n_shards, out));
        // ---- record: is one segment the extension?  (then the passes MAY be better pipelined: the other pass's front beside it)
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call0).count();
        std::lock_guard<std::mutex> lk(idx->mu);
        const asgart_stats &stt = idx->ctx[idx->last_ctx].stats;
        asgart_index::FuseVerdict &v = idx->fuse_verdict;
        if (!v.matches(settings, n_passes, modes_sig, shard, n_shards)) v.reset_for(settings, n_passes, modes_sig, shard, n_shards);
        const bool pole = n_shards == 1 && stt.passes == (uint64_t)n_passes && stt.ms_extend > 0.0 &&
                          stt.ms_longest_segment * 100.0 > stt.ms_extend * (double)idx->opt.fuse_pole_pct;
        v.note_fused(ms, stt.split_refused != 0, pole);
        if (idx->opt.debug)
            fprintf(stderr, "[asgart] passes as one job, %.1f ms: longest segment %.1f ms of %.1f ms of extension%s\n", ms,
                    stt.ms_longest_segment, stt.ms_extend, pole ? " -> timed against pipelined calls" : "");
        return 0;
    }
    // (the pipelined way was the verdict's choice: run, and record where the call returns)
    TimedPipelined timed{idx, may_pipeline};
    const int32_t rc = passes_pipelined(idx, chunks, n_chunks, settings, n_passes, shard, n_shards, out);
    timed.ok = rc == 0;
    return rc;
}

}  // extern "C"
