// call_setup.hpp -- stages setup and set_window of a search call.
// Part of pipeline.hip, the one translation unit that launches the search kernels (search_call.hpp has the stage list).
#pragma once
#include "search_call.hpp"

namespace asgart {

// ---- chunk table, probe numbering, own range -------------------------------------------------------------------------
template <class SlotT>
int32_t SearchCall<SlotT>::setup() {
    // ---- chunk table -------------------------------------------------------
    // (in the call context's pinned control block: [counters | 32 scalars | start[nc] | len[nc] | pbase[nc + 1]])
    ch_bytes = (size_t)n_chunks * 16 + ((size_t)n_chunks + 1) * 4;
    void *ctl_p = nullptr;
    RC_TRY(cx.ctl(kCtrBytes + ch_bytes + 256 + 64 + kSplitMirror, &ctl_p));
    h_ctr = static_cast<unsigned long long *>(ctl_p);
    h_scalar = h_ctr + CT_COUNT;  // source of small host-to-device updates
    h_start = reinterpret_cast<uint64_t *>(static_cast<char *>(ctl_p) + kCtrBytes + 256);
    h_len = h_start + n_chunks;
    h_pbase = reinterpret_cast<uint32_t *>(h_len + n_chunks);
    h_split = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(h_pbase + n_chunks + 1) + 63u) & ~(uintptr_t)63u);
    const uint64_t text_end = (idx->h_tail.size() && idx->h_tail.back() == '$') ? n - 1 : n;
    // probes of the chunk list, counted from the start of a pass (every pass walks the same list)
    lp.assign((size_t)n_chunks_pass + 1, 0u);
    {
        uint64_t P64 = 0;
        for (int64_t c = 0; c < n_chunks_pass; ++c) {
            const uint64_t c_start = chunks[2 * c], c_len = chunks[2 * c + 1];
            if (c_start > text_end || c_len > text_end - c_start) {
                set_error("chunk %lld = (%llu, %llu) exceeds the text (%llu bases before '$')",
                          (long long)c, (unsigned long long)c_start, (unsigned long long)c_len, (unsigned long long)text_end);
                return ASGART_E_ARG;
            }
            lp[(size_t)c] = (uint32_t)P64;
            P64 += probes_in_chunk(c_len, k, step, st->min_duplication_length);
            if (P64 * (uint64_t)n_passes >= 0xFFFFFF00ull) {
                set_error("more than 2^32 probes in one call");
                return ASGART_E_CAP;
            }
        }
        lp[(size_t)n_chunks_pass] = (uint32_t)P64;
    }
    Ppass = lp[(size_t)n_chunks_pass];
    P = Ppass * (uint32_t)n_passes;
    cx.last_P = P;
    memset(&cx.stats, 0, sizeof(cx.stats));
    cx.stats.probes_total = P;
    if (fam_out)
        for (int32_t p = 0; p < n_passes; ++p) {
            fams[p]->fam_offsets.assign(1, 0);
            fams[p]->fam_keys.clear();
            fams[p]->sds.clear();
        }
    if (want_csr) {
        status_out->assign(P, 0);
        rowoff_out->assign((size_t)P + 1, 0);
        hits_out->clear();
    }
    if (P == 0 || n_chunks == 0) return 0;  // (nothing_to_do stays set)
    if (want_csr && (n_shards != 1 || n_passes != 1)) {
        set_error("asgart_probe_hits is one unsharded pass");
        return ASGART_E_ARG;
    }
    // Multi-GPU sharding: shard r owns the automaton segments that START in the r-th slice of EVERY pass's probe
    // sequence (chunk order inside each pass as in src/bin/asgart.rs:201-253).  It computes, per pass, probe-search over
    // that slice plus a look-back halo (to decide whether its first probes continue an earlier segment) and a look-ahead
    // halo (to finish segments that run past the slice): one WINDOW per pass, all passes' windows as ONE job -- one front,
    // one launch per extension tier.  No data is exchanged between shards.
    own_lo = (uint32_t)((uint64_t)Ppass * (uint64_t)shard / (uint64_t)n_shards);  // (from the start of a pass)
    own_hi = (uint32_t)((uint64_t)Ppass * (uint64_t)(shard + 1) / (uint64_t)n_shards);
    if (own_lo == own_hi) return 0;  // (nothing_to_do stays set)
    look_back = (uint64_t)opt.shard_lookback;
    look_ahead = opt.shard_lookahead > 0 ? (uint64_t)opt.shard_lookahead
                                                  : std::max<uint64_t>(65536, (own_hi - own_lo) / 16);
    // The chunks a window can touch: c0 .. c1 of the list (a segment ends with its chunk).  The call numbers its probes
    // VIRTUALLY (RunParams): these chunks keep their probes, the others are empty in the table it uploads -- pass p's kept
    // probes are [p * K, (p + 1) * K), so probe g of the call is the (lo_lim + g - p * K)-th of pass p = g / K.
    const int64_t c0 = (int64_t)(std::upper_bound(lp.begin(), lp.end(), own_lo) - lp.begin()) - 1;
    const int64_t c1 = (int64_t)(std::upper_bound(lp.begin(), lp.end(), own_hi - 1u) - lp.begin()) - 1;
    lo_lim = lp[(size_t)c0];
    hi_lim = lp[(size_t)c1 + 1];
    K = hi_lim - lo_lim;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t cl = c % n_chunks_pass, p = c / n_chunks_pass;
        h_start[c] = chunks[2 * cl];
        h_len[c] = chunks[2 * cl + 1];
        h_pbase[c] = (uint32_t)p * K + (std::min(std::max(lp[(size_t)cl], lo_lim), hi_lim) - lo_lim);
    }
    h_pbase[n_chunks] = (uint32_t)n_passes * K;
    // what a remembered verdict about a cut segment belongs to: the settings and the chunk list (probe numbers mean nothing
    // under another step, minimum length or list)
    call_sig = 1469598103934665603ull;
    {
        auto mix = [&](uint64_t v) { call_sig = (call_sig ^ v) * 1099511628211ull; };
        mix(k);
        mix(st->max_gap_size);
        mix(st->min_duplication_length);
        mix(st->max_cardinality);
        for (int64_t c = 0; c < 2 * n_chunks_pass; ++c) mix(chunks[c]);
    }
    RC_TRY(w.chunks.reserve(ch_bytes));
    d_start = w.chunks.as<uint64_t>();
    d_len = d_start + n_chunks;
    d_pbase = reinterpret_cast<uint32_t *>(d_len + n_chunks);
    HIP_TRY(hipMemcpyAsync(d_start, h_start, ch_bytes, hipMemcpyHostToDevice, s));  // same layout on the device
    t_host0 = std::chrono::steady_clock::now();
    nothing_to_do = false;
    return 0;
}

// ---- the windows of this attempt ---------------------------------------------------------------------------------------
template <class SlotT>
void SearchCall<SlotT>::set_window() {
    // the window of a pass, counted from the start of the pass
    const uint32_t w_lo = (uint32_t)std::max<uint64_t>(lo_lim, own_lo > look_back ? own_lo - look_back : 0);
    const uint32_t w_hi = (uint32_t)std::min<uint64_t>(hi_lim, (uint64_t)own_hi + look_ahead);
    rp.init_unknown = w_lo != lo_lim ? 1u : 0u;
    rp.ch = ChunkTable{d_start, d_len, d_pbase, (int)n_chunks};
    rp.win_len = w_hi - w_lo;
    rp.win_stride = K;
    rp.g_lo = w_lo - lo_lim;
    rp.g_hi = rp.g_lo + ((uint32_t)n_passes - 1u) * K + rp.win_len;
    rp.own_off_lo = own_lo - w_lo;
    rp.own_off_hi = own_hi - w_lo;
    W = rp.g_hi - rp.g_lo;                     // extent of the per-probe arrays
    W_probes = (uint32_t)n_passes * rp.win_len;  // probes the call computes
    rp.k = (int)k;
    rp.step = (int)step;
    rp.G = st->max_gap_size;
    rp.tstar = (uint32_t)((st->max_gap_size + step - 1) / step);
    if (rp.tstar == 0) rp.tstar = 1;
    rp.M = st->min_duplication_length;
    rp.C = st->max_cardinality > 0xFFFFFF00ull ? 0xFFFFFF00u : (uint32_t)st->max_cardinality;
    rp.n_passes = (uint32_t)n_passes;
    rp.pass_chunks = (uint32_t)n_chunks_pass;
    rp.modes = 0;
    rp.blank = 0;
    for (int p = 0; p < 4; ++p) {
        rp.pbits[p] = nullptr;
        if (p >= n_passes) continue;
        const uint32_t mode = mode_of_settings(sts[p]);
        rp.modes |= (uint32_t)mode << (8 * p);
        rp.pbits[p] = opt.posbits ? idx->d_pbits[mode] : nullptr;
        if (rp.pbits[p] && idx->pbits_uses[mode] == 0) rp.blank |= 1u << p;  // (this call finds them all ones)
    }
    cx.last_rp = rp;
    cx.has_last = false;

}

}  // namespace asgart
