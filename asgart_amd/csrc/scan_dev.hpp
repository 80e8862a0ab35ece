// scan_dev.hpp -- row offsets of the hit rows and the starts of the segments, from the per-probe kept counts.
//
//   ScanEl, scan_combine      the monoid that is scanned: hits so far, the quiet run, what is known about its beginning
//   scan_publish, scan_peek   the tile descriptors of the decoupled look-back
//   scan_starts_with_resets   the start decision in a round that holds a chunk start (out of line)
//   scan_segments_kernel      the one kernel: persistent workgroups, tiles of kScanTile probes in ticket order
#pragma once

#include "device_base.hpp"

namespace asgart {

// ---------------------------------------------------------------- K2 ---------
// Row offsets and segmentation: ONE pass over the per-probe hit counts (scan_segments_kernel).
//
// What is scanned, per probe, is a small monoid: the running CSR offset (hits) and "quiet processed probes since the last
// hit-probe, reset at chunk starts" (c, flags) -- a segment starts at a hit-probe preceded by t* quiet probes or by its
// chunk's start.  A window that starts mid-chunk (sharded calls) begins with a reset of its own, marked
// "unknown": what the automaton held in front of it is not known, and stays unknown until the first hit-probe or real
// chunk start behind it.
// Single pass with decoupled look-back: persistent workgroups take tiles of kScanTile probes in ticket order; a tile's
// counts are loaded once (16 loads per lane in flight together), its aggregate is published, the exclusive prefix is
// assembled from the predecessors' published aggregates / prefixes, and the tile is walked again -- row offsets written,
// segment starts decided.  A wave owns 1024 consecutive probes as 16 rounds of 64, and everything a round needs about
// its neighbours comes out of three ballots (hit, quiet, reset) by bit arithmetic.  The round-5 version (reduce, mid, down: three kernels, every tile staged through LDS and
// walked item by item per thread) streamed 1.2 TB/s; this one is bound by its 12 bytes per probe.
struct ScanEl {
    unsigned long long hits;
    uint32_t c;      // processed probes after the last hit-probe (or all, if none)
    uint32_t flags;  // bit0 = contains a hit-probe, bit1 = contains a reset (chunk start / window start), bit2 = the LAST
                     // reset is a window start in mid-chunk (the combine below hands it on with the reset it belongs to)
};
// "no hit-probe since a window started in mid-chunk": c is only a lower bound of the quiet run
__device__ inline bool scan_unknown(const ScanEl &e) { return (e.flags & 5u) == 4u; }

__device__ inline ScanEl scan_identity() { return ScanEl{0ull, 0u, 0u}; }

__device__ inline ScanEl scan_combine(const ScanEl &a, const ScanEl &b) {
    ScanEl r;
    r.hits = a.hits + b.hits;
    if (b.flags & 2u) {
        r.c = b.c;
        r.flags = b.flags;
    } else if (b.flags & 1u) {
        r.c = b.c;
        r.flags = a.flags | 1u;
    } else {
        r.c = a.c + b.c;
        r.flags = a.flags;
    }
    return r;
}


constexpr int kScanBlock = 512;
constexpr int kScanRounds = 16;                                  // rounds of 64 probes per wave and tile
constexpr int kScanWaveSpan = 64 * kScanRounds;                  // probes a wave owns in a tile
constexpr int kScanTile = kScanWaveSpan * (kScanBlock / 64);     // 8192 probes
constexpr int kStartCap = kScanTile + kScanTile / 4;             // segment starts buffered per workgroup (a tile adds <= kScanTile)

// Tile descriptors of the look-back: two 64-bit words per tile, each carrying the descriptor's status in its top two bits
// (0 nothing, 1 the tile's own aggregate, 2 its inclusive prefix), written and read with relaxed device-scope atomics -- a
// reader that finds the two words in different states (a prefix overwriting an aggregate) reads again.
//   w0 = status << 62 | flags << 32 | c         w1 = status << 62 | hits (< 2^62)
constexpr unsigned long long kScanAgg = 1ull, kScanPre = 2ull;
__device__ inline void scan_publish(unsigned long long *desc, unsigned long long tile, unsigned long long status, const ScanEl &e) {
    __hip_atomic_store(&desc[2 * tile], status << 62 | (unsigned long long)e.flags << 32 | e.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&desc[2 * tile + 1], status << 62 | e.hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// -> status (0: not there yet, or caught between two states)
__device__ inline uint32_t scan_peek(const unsigned long long *desc, unsigned long long tile, ScanEl &e) {
    const unsigned long long w0 = __hip_atomic_load(&desc[2 * tile], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long w1 = __hip_atomic_load(&desc[2 * tile + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((w0 >> 62) != (w1 >> 62)) return 0u;
    e.hits = w1 & ((1ull << 62) - 1ull);
    e.c = (uint32_t)w0;
    e.flags = (uint32_t)(w0 >> 32) & 7u;
    return (uint32_t)(w0 >> 62);
}

__device__ inline ScanEl shfl_el(const ScanEl &e, int src) {
    ScanEl r;
    r.hits = __shfl(e.hits, src);
    r.c = __shfl(e.c, src);
    r.flags = __shfl(e.flags, src);
    return r;
}
__device__ inline ScanEl shfl_up_el(const ScanEl &e, int d) {
    ScanEl r;
    r.hits = __shfl_up(e.hits, d);
    r.c = __shfl_up(e.c, d);
    r.flags = __shfl_up(e.flags, d);
    return r;
}

// masks of the lanes above / from a lane on (l in 0..63; l = -1: every lane)
__device__ inline unsigned long long lanes_above(int l) { return l < 0 ? ~0ull : (l >= 63 ? 0ull : ~((2ull << l) - 1ull)); }
__device__ inline unsigned long long lanes_from(int l) { return l <= 0 ? ~0ull : ~((1ull << l) - 1ull); }

// The start decision of one hit-probe in a round that holds a chunk start (or the reset of a window that starts in
// mid-chunk): rare, and kept out of line -- the rounds of a tile are unrolled (their counts sit in registers).
__device__ __noinline__ void scan_starts_with_resets(bool hit, unsigned long long hm, unsigned long long qm, unsigned long long rm,
                                                     bool syn, uint32_t run_c, uint32_t run_flags, uint32_t tstar, bool &start,
                                                     bool &amb) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull, le_mask = lt_mask | (1ull << lane);
    start = amb = false;
    if (!hit) return;
    const unsigned long long rb = rm & le_mask;
    const int lr = rb ? 63 - __clzll((long long)rb) : -1;         // the last reset at or in front of this probe
    const unsigned long long hb = hm & lt_mask & lanes_from(lr);  // hit-probes in front of it, not before that reset
    const int lh = hb ? 63 - __clzll((long long)hb) : -1;
    bool has_before, unknown;
    uint32_t quiet;
    if (lh >= 0) {
        has_before = true;
        unknown = false;
        quiet = (uint32_t)__popcll(qm & lt_mask & lanes_above(lh));
    } else if (lr >= 0) {
        has_before = false;
        unknown = syn && lr == 0 && lane != 0u;  // (behind the window's own reset, no hit-probe since)
        quiet = (uint32_t)__popcll(qm & lt_mask & lanes_from(lr));
        if (unknown) has_before = true;  // (it may have one: decided by the quiet run, or not at all)
    } else {
        has_before = (run_flags & 1u) != 0u;
        unknown = (run_flags & 5u) == 4u;
        quiet = run_c + (uint32_t)__popcll(qm & lt_mask);
        if (unknown) has_before = true;
    }
    amb = unknown && quiet < tstar;
    start = !has_before || quiet >= tstar;
}

__global__ __launch_bounds__(kScanBlock) void scan_segments_kernel(RunParams rp, const uint32_t *__restrict__ p_filt,
                                                                   unsigned long long *__restrict__ desc, uint32_t n_tiles,
                                                                   unsigned long long *__restrict__ row_off,
                                                                   uint32_t *__restrict__ seg_list,
                                                                   unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t s_f[kScanTile];         // the tile's counts (every wave its own span: both passes read them from here)
    __shared__ ScanEl s_wave[kScanBlock / 64];  // the waves' aggregates of the tile
    __shared__ ScanEl s_excl;                   // the tile's exclusive prefix
    __shared__ uint32_t s_tile;
    __shared__ uint32_t s_start[kStartCap];
    __shared__ uint32_t s_nstart;
    __shared__ unsigned long long s_gbase;
    __shared__ unsigned long long sh_stat[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    if (tid < 4) sh_stat[tid] = 0;
    if (tid == 0) s_nstart = 0;
    const bool small_counts = rp.C < (1u << 25);
    unsigned long long st_n = 0, st_card = 0, st_hit = 0, st_valid = 0;  // (wave-uniform: popcounts of ballots)
    // (block-uniform) append the collected segment starts: order is irrelevant, families are sorted by (start probe,
    // ordinal) afterwards
    auto flush_starts = [&]() {
        const uint32_t ns = s_nstart;
        if (ns) {
            if (tid == 0) s_gbase = atomicAdd(&ctr[CT_SEG], (unsigned long long)ns);
            __syncthreads();
            const unsigned long long gb = s_gbase;
            for (uint32_t idx = tid; idx < ns; idx += kScanBlock) seg_list[gb + idx] = s_start[idx];
            __syncthreads();
            if (tid == 0) s_nstart = 0;
            __syncthreads();
        }
    };
    __syncthreads();
    for (;;) {
        if (tid == 0) s_tile = (uint32_t)atomicAdd(&ctr[CT_SCAN_TICKET], 1ull);  // tiles in ticket order: every predecessor
        __syncthreads();                                                          // of a tile belongs to a running workgroup
        const uint32_t tile = s_tile;
        if (tile >= n_tiles) break;
        uint32_t g_end;
        const uint32_t tile_g0 = rp.tile_of(tile, (uint32_t)kScanTile, g_end);
        const uint32_t wg0 = tile_g0 + wave * (uint32_t)kScanWaveSpan;  // this wave's first probe
        const bool syn_first = rp.init_unknown && tile_g0 + rp.win_len == g_end && wave == 0u;  // (a window that starts mid-chunk)
        // ---- the tile's counts: 16 coalesced loads per lane, all in flight together ----------------------------------
        {
            uint32_t f[kScanRounds];
#pragma unroll
            for (int r = 0; r < kScanRounds; ++r) {
                const uint32_t g = wg0 + (uint32_t)r * 64u + lane;
                f[r] = g < g_end ? p_filt[g] : kSkipN;  // (behind the window's end: nothing)
            }
#pragma unroll
            for (int r = 0; r < kScanRounds; ++r) s_f[wave * (uint32_t)kScanWaveSpan + (uint32_t)r * 64u + lane] = f[r];
        }
        // the chunk starts of this wave's span, round by round: a scalar cursor over the (few) chunks
        int c_first = chunk_of_uniform(rp.ch, wg0);
        if (rp.ch.pbase[c_first] < wg0 || rp.ch.pbase[c_first + 1] == rp.ch.pbase[c_first]) {  // next non-empty chunk that starts at or behind wg0
            ++c_first;
            while (c_first < rp.ch.n_chunks && rp.ch.pbase[c_first + 1] == rp.ch.pbase[c_first]) ++c_first;
        }
        const uint32_t pb_first = c_first < rp.ch.n_chunks ? rp.ch.pbase[c_first] : 0xFFFFFFFFu;
        // first probes of chunks in [ga, ga + 64): cn / pb = the next chunk that has not started yet and its first probe
        auto resets_of = [&](int &cn, uint32_t &pb, uint32_t ga) -> unsigned long long {
            unsigned long long m = 0;
            while (pb < ga + 64u && pb < g_end) {  // (pb = ~0u once the table is exhausted)
                const uint32_t pb_next = rp.ch.pbase[cn + 1];             // (the table has n_chunks + 1 entries)
                if (pb_next > pb) m |= 1ull << (pb - ga);                 // (only non-empty chunks have a first probe)
                ++cn;
                pb = cn < rp.ch.n_chunks ? pb_next : 0xFFFFFFFFu;
            }
            return m;
        };
        // one round's element: what it adds to a running (c, flags)
        auto round_el = [&](unsigned long long hm, unsigned long long qm, unsigned long long rm, bool syn) -> ScanEl {
            ScanEl e{0ull, 0u, 0u};
            const int lh = hm ? 63 - __clzll((long long)hm) : -1, lr = rm ? 63 - __clzll((long long)rm) : -1;
            if (lr >= 0) {
                const bool hit_since = lh >= lr;
                e.c = (uint32_t)__popcll(qm & (hit_since ? lanes_above(lh) : lanes_from(lr)));
                e.flags = 2u | (hit_since ? 1u : 0u) | ((syn && lr == 0) ? 4u : 0u);
            } else if (lh >= 0) {
                e.c = (uint32_t)__popcll(qm & lanes_above(lh));
                e.flags = 1u;
            } else {
                e.c = (uint32_t)__popcll(qm);
            }
            return e;
        };
        // ---- pass 1: the wave's aggregate -------------------------------------------------------------------------------
        ScanEl agg = scan_identity();
        unsigned long long vsum = 0;
        {
            int cn = c_first;
            uint32_t pb = pb_first;
#pragma unroll 1
            for (int r = 0; r < kScanRounds; ++r) {
                const uint32_t fr = s_f[wave * (uint32_t)kScanWaveSpan + (uint32_t)r * 64u + lane];
                const bool hit = fr >= 1u && fr < kPending;
                const unsigned long long hm = __ballot(hit), qm = __ballot(fr == 0u);
                unsigned long long rm = resets_of(cn, pb, wg0 + (uint32_t)r * 64u);
                const bool syn = syn_first && r == 0;
                if (syn) rm |= 1ull;
                vsum += hit ? fr : 0u;
                const ScanEl e = round_el(hm, qm, rm, syn);
                agg = scan_combine(agg, e);
            }
            for (int off = 32; off > 0; off >>= 1) vsum += __shfl_down(vsum, off);
            agg.hits = __shfl(vsum, 0);
        }
        if (lane == 0) s_wave[wave] = agg;
        __syncthreads();
        // ---- the tile's aggregate is published, its exclusive prefix assembled from its predecessors' (wave 0) --------
        if (wave == 0) {
            ScanEl tile_agg = scan_identity();
            for (int w = 0; w < kScanBlock / 64; ++w) tile_agg = scan_combine(tile_agg, s_wave[w]);
            ScanEl excl = scan_identity();
            if (tile == 0) {
                if (lane == 0) scan_publish(desc, 0, kScanPre, tile_agg);
            } else {
                if (lane == 0) scan_publish(desc, tile, kScanAgg, tile_agg);
                // windows of 64 predecessors, nearest first: lane l looks at tile `hi - 64 + l` (lane 63 = the nearest)
                ScanEl acc = scan_identity();  // combination of the tiles [hi, tile)
                long long hi = tile;
                for (;;) {
                    const long long t_l = hi - 64 + (long long)lane;
                    ScanEl e = scan_identity();
                    uint32_t stt = 3u;  // (no such tile: identity, never waited for)
                    if (t_l >= 0) stt = scan_peek(desc, (unsigned long long)t_l, e);
                    const unsigned long long pm = __ballot(stt == (uint32_t)kScanPre), zm = __ballot(stt == 0u);
                    const int pl = pm ? 63 - __clzll((long long)pm) : -1;  // the nearest tile whose inclusive prefix is known
                    if (zm & lanes_above(pl)) {  // a tile between it and us has not published yet
                        __builtin_amdgcn_s_sleep(2);
                        continue;
                    }
                    if ((int)lane < pl || stt == 3u) e = scan_identity();
                    // ordered combination of the lanes pl .. 63 (an inclusive scan; lane 63 holds the result)
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const ScanEl o = shfl_up_el(e, d);
                        if ((int)lane >= d) e = scan_combine(o, e);
                    }
                    acc = scan_combine(shfl_el(e, 63), acc);
                    if (pl >= 0 || hi - 64 <= 0) break;
                    hi -= 64;
                }
                excl = acc;
                if (lane == 0) scan_publish(desc, tile, kScanPre, scan_combine(excl, tile_agg));
            }
            if (lane == 0) {
                s_excl = excl;
                if (tile + 1u == n_tiles) ctr[CT_TOTAL_HITS] = excl.hits + tile_agg.hits;
            }
        }
        __syncthreads();
        // ---- pass 2: row offsets and segment starts (the counts come back from LDS: this loop is not unrolled) -----------
        ScanEl run = s_excl;
        for (uint32_t w = 0; w < wave; ++w) run = scan_combine(run, s_wave[w]);
        {
            int cn = c_first;
            uint32_t pb = pb_first;
            // this call's own range of the tile's window, as probe numbers (wave-uniform)
            const uint32_t own_lo_g = g_end - rp.win_len + rp.own_off_lo, own_hi_g = g_end - rp.win_len + rp.own_off_hi;
#pragma unroll 1
            for (int r = 0; r < kScanRounds; ++r) {
                const uint32_t ga = wg0 + (uint32_t)r * 64u, g = ga + lane;
                const uint32_t fr = s_f[wave * (uint32_t)kScanWaveSpan + (uint32_t)r * 64u + lane];
                const uint32_t n_valid = ga < g_end ? min(64u, g_end - ga) : 0u;  // (lanes behind the window's end hold kSkipN)
                const bool hit = fr >= 1u && fr < kPending;
                const unsigned long long hm = __ballot(hit), qm = __ballot(fr == 0u), cardm = __ballot(fr == kSkipCard);
                unsigned long long rm = resets_of(cn, pb, ga);
                const bool syn = syn_first && r == 0;
                if (syn) rm |= 1ull;
                // statistics (of the window's probes): a probe is a hit-probe, quiet, skipped for its cardinality or for its N
                const uint32_t n_hit = (uint32_t)__popcll(hm), n_card = (uint32_t)__popcll(cardm);
                st_valid += n_valid;
                st_hit += n_hit;
                st_card += n_card;
                st_n += n_valid - n_hit - n_card - (uint32_t)__popcll(qm);
                // row offsets: exclusive prefix of the hit counts (a count is at most max_cardinality: one 32-bit scan while
                // 64 of them fit, else two 16-bit halves)
                const uint32_t v = hit ? fr : 0u;
                unsigned long long incl;
                if (small_counts) {
                    incl = wave_incl_scan(v);
                } else {
                    const uint32_t lo16 = wave_incl_scan(v & 0xFFFFu), hi16 = wave_incl_scan(v >> 16);
                    incl = (unsigned long long)lo16 + ((unsigned long long)hi16 << 16);
                }
                if (lane < n_valid) row_off[g] = run.hits + incl - v;
                // (the row offset behind a window's last probe: what the CSR holds up to there)
                if (lane + 1u == n_valid && g + 1u == g_end) row_off[g_end] = run.hits + incl;
                // segment starts: a hit-probe of this call's own range with no hit-probe in front of it since its chunk
                // started, or with t* quiet probes in between.  (A window's first probe is never owned when the window
                // starts in mid-chunk: the look-back halo is at least one probe.)
                const uint32_t l_lo = own_lo_g > ga ? min(own_lo_g - ga, 64u) : 0u, l_hi = own_hi_g > ga ? min(own_hi_g - ga, 64u) : 0u;
                const unsigned long long ownm = (l_hi >= 64u ? ~0ull : (1ull << l_hi) - 1ull) & ~(l_lo >= 64u ? ~0ull : (1ull << l_lo) - 1ull);
                unsigned long long sm = 0, ambm = 0;
                if (hm & ownm) {
                    if (!rm) {
                        // no chunk starts in the round (all but a handful): the quiet probes below a lane, and -- by an inclusive
                        // max-scan over the hit lanes, whose counts ascend -- the count at the last hit-probe in front of it
                        const uint32_t Q = __builtin_amdgcn_mbcnt_hi((uint32_t)(qm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qm, 0u));
                        uint32_t xp = __shfl_up(wave_incl_max_scan(hit ? Q + 1u : 0u), 1);
                        if (lane == 0u) xp = 0u;
                        const bool has_in = xp != 0u;                                       // a hit-probe in front of it in this round
                        const bool unknown = !has_in && scan_unknown(run);
                        const bool has_before = has_in || (run.flags & 1u) != 0u || unknown;  // (unknown: it may have one)
                        const uint32_t quiet = has_in ? Q - (xp - 1u) : run.c + Q;
                        sm = __ballot(hit && (!has_before || quiet >= rp.tstar)) & ownm;
                        ambm = __ballot(hit && unknown && quiet < rp.tstar) & ownm;
                    } else {
                        bool start = false, amb = false;
                        scan_starts_with_resets(hit, hm, qm, rm, syn, run.c, run.flags, rp.tstar, start, amb);
                        sm = __ballot(start) & ownm;
                        ambm = __ballot(amb) & ownm;
                    }
                }
                if (ambm && lane == 0u) atomicAdd(&ctr[CT_AMBIG], (unsigned long long)__popcll(ambm));
                if (sm) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&s_nstart, (uint32_t)__popcll(sm));
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    if ((sm >> lane) & 1ull) s_start[base + (uint32_t)__popcll(sm & lt_mask)] = g;
                }
                ScanEl e = round_el(hm, qm, rm, syn);
                e.hits = __shfl(incl, 63);
                run = scan_combine(run, e);
            }
        }
        __syncthreads();  // (s_tile, s_wave, s_excl are rewritten by the next tile)
        if (s_nstart > (uint32_t)(kStartCap - kScanTile)) flush_starts();
    }
    flush_starts();
    if (lane == 0) {
        atomicAdd(&sh_stat[0], st_n);
        atomicAdd(&sh_stat[1], st_card);
        atomicAdd(&sh_stat[2], st_hit);
        atomicAdd(&sh_stat[3], st_valid);
    }
    __syncthreads();
    if (tid == 0) {
        if (sh_stat[0]) atomicAdd(&ctr[CT_N_SKIPPED], sh_stat[0]);
        if (sh_stat[1]) atomicAdd(&ctr[CT_CARD_SKIPPED], sh_stat[1]);
        if (sh_stat[2]) atomicAdd(&ctr[CT_WITH_HITS], sh_stat[2]);
        if (sh_stat[3] > sh_stat[0]) atomicAdd(&ctr[CT_SEARCHED], sh_stat[3] - sh_stat[0]);
    }
}

}  // namespace asgart
