// call_front.hpp -- stages front and csr_out of a search call, and the per-probe workspace they work in.
// Part of pipeline.hip, the one translation unit that launches the search kernels (search_call.hpp has the stage list).
#pragma once
#include "search_call.hpp"

namespace asgart {

// Test hook (option test_stall_s): a kernel that does nothing for that many seconds on the call's main stream, so
// that the watchdog's way out of a stuck device can be exercised (wall_clock64 ticks at 100 MHz).
__global__ void stall_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(100);
}

// The per-probe buffers of a call context for a window of W probes, and their sizes (n_blk: every window of a call ends
// with a partial tile).  reserve_probe_workspace and carve_probe_workspace read this table and nothing else.
struct ProbeBuffer {
    DevBuf Workspace::*buf;
    size_t (*bytes)(uint64_t W, bool wide);
};
static const ProbeBuffer kProbeBuffers[7] = {
    {&Workspace::p_lo, [](uint64_t W, bool wide) { return (size_t)W * (wide ? 8 : 4); }},
    {&Workspace::p_raw, [](uint64_t W, bool) { return (size_t)W * 4; }},
    {&Workspace::p_filt, [](uint64_t W, bool) { return (size_t)W * 4; }},
    {&Workspace::row_off, [](uint64_t W, bool) { return ((size_t)W + 1) * 8; }},
    {&Workspace::blk, [](uint64_t W, bool) { return (size_t)((W + kScanTile - 1) / kScanTile + 4) * sizeof(ScanEl); }},
    {&Workspace::big_list, [](uint64_t W, bool) { return (size_t)W * 4; }},
    {&Workspace::rank_list, [](uint64_t W, bool) { return (size_t)W * 4; }},  // (reserved only with d_sap, always carved)
};

int32_t reserve_probe_workspace(asgart_index *idx, SearchCtx &cx, uint64_t W) {
    Workspace &w = cx.ws;
    for (const ProbeBuffer &pb : kProbeBuffers)
        if (pb.buf != &Workspace::rank_list || idx->d_sap) RC_TRY((w.*pb.buf).reserve(pb.bytes(W, idx->wide)));
    RC_TRY(w.counters.reserve(CT_COUNT * 8));
    return 0;
}

// On the slow boxes of the pool every first allocation costs ~30 ms per GiB: the nine buffers of 1-5 GB that the two
// contexts' workspace used to allocate at asgart_index_prepare were 0.8 s of a cold run there.  The sorter's key
// buffers (n 64-bit words each) are in the block cache at that moment: one of them holds both contexts' workspace.
bool carve_probe_workspace(asgart_index *idx, const uint64_t *Wc) {
    if (idx->ws_arena.p) return false;
    size_t off = 0;
    struct Piece {
        DevBuf *b;
        size_t off, bytes;
    };
    std::vector<Piece> pieces;
    for (int c = 0; c < kNumCtx; ++c)
        for (const ProbeBuffer &pb : kProbeBuffers) {
            DevBuf &b = idx->ctx[c].ws.*pb.buf;
            if (b.p) return false;  // (something is reserved already: leave everything as it is)
            const size_t sz = (pb.bytes(Wc[c], idx->wide) + 4095) & ~(size_t)4095;
            pieces.push_back(Piece{&b, off, sz});
            off += sz;
        }
    size_t cap = 0;
    void *p = BlockCache::take(off, &cap, 30);
    if (!p) return false;
    idx->ws_arena.p = p;
    idx->ws_arena.cap = cap;
    for (const Piece &pc : pieces) {
        pc.b->p = static_cast<char *>(p) + pc.off;
        pc.b->cap = pc.bytes;
        pc.b->view = true;
    }
    return true;
}

// ---- probe search, row offsets + segment starts, hit rows (*ambiguous: a start decision needs a longer look-back) ----------
template <class SlotT>
int32_t SearchCall<SlotT>::front(bool *ambiguous) {
    // ---- workspace (indexed by absolute probe number through shifted pointers) ---
    const uint32_t n_blk = rp.n_tiles((uint32_t)kScanTile);
    const uint64_t seg_cap = (uint64_t)W_probes / (rp.tstar + 1) + (uint64_t)n_chunks + 64;
    RC_TRY(reserve_probe_workspace(idx, cx, W));
    RC_TRY(w.seg_list.reserve((size_t)seg_cap * 4));
    RC_TRY(w.counters.reserve(CT_COUNT * 8));
    d_ctr = w.counters.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(d_ctr, 0, CT_COUNT * 8, s));
    ix = idx->template view<SlotT>();
    p_lo = w.p_lo.as<SlotT>() - rp.g_lo;
    p_raw = w.p_raw.as<uint32_t>() - rp.g_lo;
    p_filt = w.p_filt.as<uint32_t>() - rp.g_lo;
    row_off = w.row_off.as<unsigned long long>() - rp.g_lo;
    unsigned long long *scan_desc = w.blk.as<unsigned long long>();  // two words per scan tile (scan_segments_kernel)
    uint32_t *big_list = w.big_list.as<uint32_t>();
    uint32_t *rank_list = w.rank_list.as<uint32_t>();
    seg_list = w.seg_list.as<uint32_t>();

    if (opt.test_stall_s > 0) stall_kernel<<<1, 64, 0, s>>>((unsigned long long)opt.test_stall_s * 100000000ull);
    // ---- K1: probe search + filtered counts -----------------------------------
    HIP_TRY(hipEventRecord(cx.ev[EV_SEARCH], s));
    probe_count_kernel<SlotT, false><<<rp.n_tiles((uint32_t)kProbeBlock), kProbeThreads, 0, s>>>(
        ix, rp, p_lo, p_raw, p_filt, big_list, rank_list, d_ctr);
    HIP_TRY(hipEventRecord(cx.ev[EV_PROBE_COUNT], s));
    collect_pending_kernel<<<std::min<uint32_t>(rp.n_tiles((uint32_t)kCollectTile), 256u * 8u), kCollectBlock, 0, s>>>(
        rp, p_filt, big_list, rank_list, d_ctr);
    big_count_kernel<SlotT, false><<<2048, 256, 0, s>>>(ix, rp, p_lo, p_raw, p_filt, big_list, d_ctr);
    // (after big_count_kernel: what it appends to big_list is for the fill only)
    // (its rows for fill_ranked_kernel: from the end of big_list's W entries downwards)
    uint32_t *const ranked_top = big_list + W;
    if (ix.sap)
        rank_count_kernel<SlotT, false><<<2048, 256, 0, s>>>(ix, rp, p_lo, p_raw, p_filt, rank_list, big_list, ranked_top,
                                                             ix.sar ? idx->ranked_fill : 0, d_ctr);
    HIP_TRY(hipEventRecord(cx.ev[EV_SEARCHED], s));
    // ---- K2: scans + segmentation ----------------------------------------------
    HIP_TRY(hipMemsetAsync(scan_desc, 0, (size_t)n_blk * 16, s));
    scan_segments_kernel<<<std::min<uint32_t>(n_blk, 256u * 2u), kScanBlock, 0, s>>>(rp, p_filt, scan_desc, n_blk, row_off, seg_list, d_ctr);
    HIP_TRY(hipEventRecord(cx.ev[EV_SCANNED], s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr, kCtrBytes, hipMemcpyDeviceToHost, s));
    RC_TRY(wd_sync(idx, cx, s, "the probe search and the scans"));
    total_hits = h_ctr[CT_TOTAL_HITS];
    n_seg = h_ctr[CT_SEG];
    if (h_ctr[CT_AMBIG]) {  // a start decision needs more history: the caller widens the look-back halo
        *ambiguous = true;
        return 0;
    }
    if (n_seg > seg_cap) {
        set_error("internal: segment list overflow (%llu > %llu)", (unsigned long long)n_seg,
                  (unsigned long long)seg_cap);
        return ASGART_E_CAP;
    }
    // ---- K3: CSR fill -----------------------------------------------------------
    // On a stream of its own (idle until the tiers are launched; the main stream has just been drained): the placement
    // walk, which reads the per-probe counts only, runs beside it -- the fill is bound by the suffix-array intervals it
    // gathers, the walk by its round trips.  Whoever needs the hit rows waits for ev[EV_HIT_ROWS].
    RC_TRY(w.hits.reserve((size_t)(total_hits + 64) * sizeof(SlotT)));
    hits = w.hits.as<SlotT>();
    hipStream_t sf = cx.fill_stream;
    HIP_TRY(hipEventRecord(cx.ev[EV_FILL], sf));
    fill_small_kernel<SlotT><<<(rp.n_tiles((uint32_t)kFillTile) + kFillWaves - 1u) / kFillWaves, 64 * kFillWaves, 0, sf>>>(
        ix, rp, p_lo, p_raw, p_filt, row_off, hits);
    if (h_ctr[CT_BIG])
        fill_big_kernel<SlotT><<<2048, 256, 0, sf>>>(ix, rp, p_lo, p_raw, p_filt, row_off, hits,
                                                     big_list, d_ctr);
    if constexpr (sizeof(SlotT) == 4) {
        if (h_ctr[CT_RANKED])
            fill_ranked_kernel<SlotT><<<(unsigned)std::min<uint64_t>((h_ctr[CT_RANKED] + 255) / 256, 4096), 256, 0, sf>>>(
                ix, rp, p_lo, p_raw, p_filt, row_off, hits, ranked_top, d_ctr);
    }
    HIP_TRY(hipEventRecord(cx.ev[EV_HIT_ROWS], sf));
    HIP_TRY(hipGetLastError());

    return 0;
}

// ---- asgart_probe_hits: the per-probe hit rows to the host ----------------------------------------------------------------
template <class SlotT>
int32_t SearchCall<SlotT>::csr_out() {
    std::vector<uint32_t> h_filt(P);
    std::vector<SlotT> h_hits((size_t)total_hits);
    RC_TRY(wd_sync(idx, cx, s, "the hit rows"));  // (the copies below go to pageable memory: they block inside the copy)
    HIP_TRY(hipMemcpyAsync(h_filt.data(), p_filt, (size_t)P * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(rowoff_out->data(), row_off, ((size_t)P + 1) * 8,
                           hipMemcpyDeviceToHost, s));
    if (total_hits)
        HIP_TRY(hipMemcpyAsync(h_hits.data(), hits, (size_t)total_hits * sizeof(SlotT),
                               hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t g = 0; g < P; ++g)
        (*status_out)[g] = h_filt[g] == kSkipN ? 1 : (h_filt[g] == kSkipCard ? 2 : 0);
    hits_out->resize((size_t)total_hits);
    for (uint64_t j = 0; j < total_hits; ++j) (*hits_out)[j] = h_hits[j];
    return 0;
}

}  // namespace asgart
