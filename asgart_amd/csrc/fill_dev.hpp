// fill_dev.hpp -- the hit rows: the filtered occurrences of every probe, in suffix-array order, into the CSR whose row
// offsets scan_dev.hpp wrote.
//
//   walk_small_rows      a wave walks 64 small intervals entry by entry, their entries spread over its lanes
//   fill_small_kernel    a wave per tile of 1024 probes: the rows of intervals of up to kSmallInterval entries
//   fill_big_kernel      a wave per 64 entries of big_list: larger intervals, streamed 256 entries per round trip
//   fill_ranked_kernel   a wave per 64 entries of the ranked list: rows of frequent k-mers from the tail of their
//                        position-sorted list (32-bit slots only)
//   fill_account_kernel  what the three served in the last call (asgart_fill_counts, asgart_fill_tally)
// The three wave-per-64-rows kernels (big_count_kernel of probe_dev.hpp, fill_big_kernel, fill_ranked_kernel) set their
// rows up alike -- lane l row e0 + l, its place by probe_at, its filter by hit_rule, thr and self broadcast per row -- and
// stream them each in its own way: the count's early exit, the fill's ballot compaction and the ranked fill's bitmap are
// measured decisions, recorded where they stand.
#pragma once

#include "device_base.hpp"

namespace asgart {

// ---- a wave walks many small suffix-array intervals entry by entry --------------------------------------------------
// A lane that walks its own interval sa[lo, lo + raw) holds one load in flight, the wave lasts as long as its longest
// interval, and the lanes without an interval idle.  Here every lane of the (whole, converged) wave brings ONE item --
// an interval of raw <= kSmallInterval entries, raw = 0: none -- and the wave processes the sum of their entries 64 at a
// time, in suffix-array order, all loads of a round in flight together:
//   * the exclusive prefix of raw over the lanes (wave scan) numbers the entries; entry e finds its owner -- the last
//     lane whose prefix is <= e -- by bisection of the prefixes (six lane reads);
//   * the owner's hit filter travels as two numbers: entry x is kept when x >= thr and x != self (HitRule);
//   * per round, round(own, r, x, keep, km) is called by all lanes: own / r = owner lane and place inside the owner's
//     interval of the entry this lane loaded, x its value, keep its predicate, km the ballot of `keep` over the round.
// fill_small_kernel places the kept entries with it: an entry's rank inside its row is the popcount of km below it inside
// its row, plus the end of the previous round's km where the row began there (a row spans at most two rounds).  No LDS,
// no atomics.
template <class SlotT, class F>
__device__ inline void walk_small_rows(const SlotT *__restrict__ sa, unsigned long long lo, uint32_t raw, HitRule hr, F &&round) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t incl = wave_incl_scan(raw), pre = incl - raw;
    const uint32_t total = lane_of(incl, 63u);
    for (uint32_t base = 0; base < total; base += 64u) {
        const uint32_t e = base + lane;
        uint32_t own = 0;
#pragma unroll
        for (uint32_t step = 32u; step; step >>= 1)
            if (lane_get(pre, own + step) <= e) own += step;  // (own + step <= 63)
        // (items without entries repeat their successor's prefix: the LAST lane with pre <= e has entries while e < total)
        const uint32_t r = e - lane_get(pre, own);
        const unsigned long long lo_o = lane_get(lo, own);
        const HitRule hr_o = lane_get(hr, own);
        const bool live = e < total;
        SlotT x = 0;
        if (live) x = sa[lo_o + r];
        const bool keep = live && hr_o.keeps(x);
        round(own, r, x, keep, (unsigned long long)__ballot(keep));
    }
}

// ---------------------------------------------------------------- K3 ---------
// Rows of small intervals.  One probe in twenty has such a row on the GRCh38-shaped input: with a thread per probe those
// few lanes gathered their three per-probe values and then walked their interval one dependent load at a time.  A wave
// now takes a tile of kFillTile probes: their p_filt words are read coalesced, all in flight; the probes with a row (f != 0
// && f < kPending) are compacted by ballots into a list in LDS; p_raw, p_lo and row_off are gathered for those only, 64 at
// a time, and the entries of their intervals are spread over the lanes (walk_small_rows), each kept entry placed by its
// rank inside its row.
constexpr int kFillTile = 1024, kFillWaves = 4;  // probes per wave; waves per workgroup
template <class SlotT>
__global__ __launch_bounds__(64 * kFillWaves) void fill_small_kernel(IndexView<SlotT> ix, RunParams rp,
                                                                     const SlotT *__restrict__ p_lo,
                                                                     const uint32_t *__restrict__ p_raw,
                                                                     const uint32_t *__restrict__ p_filt,
                                                                     const unsigned long long *__restrict__ row_off,
                                                                     SlotT *__restrict__ hits) {
    __shared__ unsigned short s_rows[kFillWaves][kFillTile];  // per wave: the tile's probes with a row (offsets from its first)
    unsigned short *const rows = s_rows[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t tile = uni(blockIdx.x * (uint32_t)kFillWaves + (threadIdx.x >> 6));
    if (tile >= rp.n_tiles((uint32_t)kFillTile)) return;  // (the whole wave; no workgroup barrier below)
    uint32_t g_end;
    const uint32_t gb = rp.tile_of(tile, (uint32_t)kFillTile, g_end);
    // (the chunk of the tile's first probe, once, in scalar registers; a lane whose probe lies behind a chunk boundary
    // steps on from there -- a tile rarely spans two chunks -- instead of bisecting the table per lane)
    const int c0 = chunk_of_uniform(rp.ch, gb);
    constexpr int kSub = kFillTile / 64;
    uint32_t f[kSub];
#pragma unroll
    for (int u = 0; u < kSub; ++u) {
        const uint32_t g = gb + (uint32_t)u * 64u + lane;
        f[u] = g < g_end ? p_filt[g] : 0u;
    }
    uint32_t n_rows = 0;
#pragma unroll
    for (int u = 0; u < kSub; ++u) {
        const bool has = f[u] != 0u && f[u] < kPending;
        const unsigned long long m = __ballot(has);
        if (has) rows[n_rows + (uint32_t)__popcll(m & lt_mask)] = (unsigned short)((uint32_t)u * 64u + lane);
        n_rows += (uint32_t)__popcll(m);
    }
    n_rows = uni(n_rows);
    wave_lds_sync();
    for (uint32_t j0 = 0; j0 < n_rows; j0 += 64u) {
        const uint32_t j = j0 + lane;
        uint32_t raw = 0;
        unsigned long long lo = 0, w = 0;
        HitRule hr = {0ull, 0ull};
        if (j < n_rows) {
            const uint32_t g = gb + rows[j];
            raw = p_raw[g];
            if (raw > (uint32_t)kSmallInterval) raw = 0;  // (fill_big_kernel's, fill_ranked_kernel's)
            lo = p_lo[g];
            w = row_off[g];
            int c = c0;
            while (c + 1 < rp.ch.n_chunks && g >= rp.ch.pbase[c + 1]) ++c;
            hr = hit_rule(probe_at(rp, c, g));
        }
        unsigned long long km_prev = 0;  // the round before (wave-uniform)
        walk_small_rows(ix.sa, lo, raw, hr,
                        [&](uint32_t own, uint32_t r, SlotT x, bool keep, unsigned long long km) {
                            // the kept entries of the row in front of this one: r entries, the last min(r, lane) of them in
                            // the lanes below, the others at the end of the round before
                            const unsigned long long w_o = lane_get(w, own);
                            if (keep) {
                                const uint32_t here = min(r, lane);
                                uint32_t rank = (uint32_t)__popcll(km & lt_mask & ~((1ull << (lane - here)) - 1ull));
                                if (r > here) rank += (uint32_t)__popcll(km_prev >> (64u - (r - here)));  // (1 <= r - here < 32)
                                hits[w_o + rank] = x;
                            }
                            km_prev = km;
                        });
    }
}

// Large intervals, one wave per 64 of them (set-up in parallel across the lanes, like the count
// kernel): ballot / prefix-popcount compaction of the kept hits, SA order kept.
template <class SlotT>
__global__ __launch_bounds__(256) void fill_big_kernel(IndexView<SlotT> ix, RunParams rp,
                                                       const SlotT *__restrict__ p_lo,
                                                       const uint32_t *__restrict__ p_raw,
                                                       const uint32_t *__restrict__ p_filt,
                                                       const unsigned long long *__restrict__ row_off,
                                                       SlotT *__restrict__ hits,
                                                       const uint32_t *__restrict__ big_list,
                                                       const unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint64_t n_big = ctr[CT_BIG];
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t e0 = wave * 64u; e0 < n_big; e0 += n_waves * 64u) {
        const uint32_t np = (uint32_t)min((uint64_t)64, n_big - e0);
        unsigned long long lo = 0, hi = 0, w0 = 0;
        HitRule hr = {0ull, 0ull};
        bool want = false;
        if (lane < np) {
            const uint32_t g = big_list[e0 + lane];
            const uint32_t f = p_filt[g];
            want = f != 0 && f < kPending;  // skipped / empty rows have nothing to fill
            if (want) {
                hr = hit_rule(probe_at(rp, g));
                lo = p_lo[g];
                hi = lo + p_raw[g];
                w0 = row_off[g];
            }
        }
        unsigned long long todo = __ballot(want);
        while (todo) {
            const uint32_t p = (uint32_t)(__ffsll((long long)todo) - 1);
            todo &= todo - 1;
            const unsigned long long lo_p = lane_of(lo, p), hi_p = lane_of(hi, p);
            const HitRule hr_p = lane_of(hr, p);
            unsigned long long w = lane_of(w0, p);
            for (unsigned long long base = lo_p; base < hi_p; base += 256) {  // four slices in flight per round trip
                SlotT x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned long long r = base + 64u * u + lane;
                    x[u] = r < hi_p ? ix.sa[r] : (SlotT)0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned long long r = base + 64u * u + lane;
                    const bool keep = r < hi_p && hr_p.keeps(x[u]);
                    const unsigned long long m = __ballot(keep);
                    if (keep) hits[w + __popcll(m & lt_mask)] = x[u];
                    w += __popcll(m);
                }
            }
        }
    }
}

// Rows of frequent k-mers, one wave per row (set-up of 64 rows side by side across the lanes, like fill_big_kernel).  The
// hit filter keeps the occurrences beyond a position threshold -- less the probe's own offset in a reversed pass -- so the
// cnt kept hits of a row are among the last cnt + 1 entries of the interval's POSITION-sorted list: those are read (with
// the suffix-array slot each came from, ix.sar) instead of the R entries of the interval, and filtered like everywhere
// else.  A row is written in suffix-array order: every kept entry sets the bit of its slot in a bitmap of the interval
// (LDS, R bits), one pass of popcounts and a wave scan turns the bitmap into the number of kept entries below each of
// its words, and an entry's place in the row is that number plus the set bits below its own in its word.  (A bitonic
// sort of the kept entries in LDS -- 45 dependent compare-exchange rounds for 512 -- took 28 us per row: 26 ms per
// GRCh38-shaped step where streaming the intervals takes 11.)  The next row's entries are in flight while a row is
// placed.  32-bit slots only.
constexpr int kRankedRounds = (kRankedCap + 1 + 63) / 64;  // loads of 64 entries that cover cnt + 1 <= kRankedCap + 1
constexpr int kRankedWords = kRankedMaxR / 32;             // bitmap words per wave
template <class SlotT>
__global__ __launch_bounds__(256) void fill_ranked_kernel(IndexView<SlotT> ix, RunParams rp,
                                                          const SlotT *__restrict__ p_lo,
                                                          const uint32_t *__restrict__ p_raw,
                                                          const uint32_t *__restrict__ p_filt,
                                                          const unsigned long long *__restrict__ row_off,
                                                          SlotT *__restrict__ hits,
                                                          const uint32_t *__restrict__ ranked_top,
                                                          const unsigned long long *__restrict__ ctr) {
    static_assert(sizeof(SlotT) == 4, "32-bit slots and positions");
    __shared__ uint32_t s_bits[4][kRankedWords];
    __shared__ unsigned short s_below[4][kRankedWords];  // (a row keeps at most kRankedCap hits)
    uint32_t *const bm = s_bits[threadIdx.x >> 6];
    unsigned short *const below = s_below[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_rk = ctr[CT_RANKED];
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t e0 = wave * 64u; e0 < n_rk; e0 += n_waves * 64u) {
        const uint32_t np = (uint32_t)min((uint64_t)64, n_rk - e0);
        unsigned long long lo = 0, a0 = 0, w0 = 0;
        HitRule hr = {0ull, 0ull};
        uint32_t cnt = 0, R = 0;
        if (lane < np) {
            const uint32_t g = *(ranked_top - 1 - (long long)(e0 + lane));
            cnt = min(p_filt[g], (uint32_t)kRankedCap);              // (1..kRankedCap: ranked_fill_takes)
            R = min(p_raw[g], (uint32_t)kRankedMaxR);                // (<= kRankedMaxR: likewise)
            hr = hit_rule(probe_at(rp, g));
            lo = p_lo[g];
            a0 = R > cnt + 1u ? lo + R - cnt - 1u : lo;
            w0 = row_off[g];
        }
        // the tail of a row's list and the slots of its entries: all rounds in flight together
        SlotT xn[kRankedRounds], sn[kRankedRounds];
        auto fetch = [&](uint32_t p) {
            const unsigned long long a0_p = lane_of(a0, p), a1_p = lane_of(lo, p) + lane_of(R, p);
#pragma unroll
            for (int u = 0; u < kRankedRounds; ++u) {
                const unsigned long long r = a0_p + 64u * u + lane;
                xn[u] = r < a1_p ? ix.sap[r] : (SlotT)0;
                sn[u] = r < a1_p ? ix.sar[r] : (SlotT)0;
            }
        };
        fetch(0u);
        for (uint32_t p = 0; p < np; ++p) {
            const unsigned long long lo_p = lane_of(lo, p), a0_p = lane_of(a0, p), w_p = lane_of(w0, p);
            const HitRule hr_p = lane_of(hr, p);
            const uint32_t cnt_p = lane_of(cnt, p), R_p = lane_of(R, p);
            const unsigned long long a1_p = lo_p + R_p;
            SlotT x[kRankedRounds];
            uint32_t rel[kRankedRounds];  // slot inside the interval; ~0u: not kept
#pragma unroll
            for (int u = 0; u < kRankedRounds; ++u) {
                const unsigned long long r = a0_p + 64u * u + lane;
                x[u] = xn[u];
                const uint32_t d = (uint32_t)sn[u] - (uint32_t)lo_p;
                rel[u] = r < a1_p && hr_p.keeps(x[u]) && d < R_p ? d : ~0u;
            }
            if (p + 1 < np) fetch(p + 1u);
            const uint32_t nw = (R_p + 31u) >> 5;
            for (uint32_t j = lane; j < nw; j += 64u) bm[j] = 0u;
            wave_lds_sync();
#pragma unroll
            for (int u = 0; u < kRankedRounds; ++u)
                if (rel[u] != ~0u) atomicOr(&bm[rel[u] >> 5], 1u << (rel[u] & 31u));
            wave_lds_sync();
            uint32_t run = 0;  // kept entries below the words of this round
            for (uint32_t base = 0; base < nw; base += 64u) {
                const uint32_t j = base + lane;
                const uint32_t c = j < nw ? (uint32_t)__popc(bm[j]) : 0u;
                const uint32_t incl = wave_incl_scan(c);
                if (j < nw) below[j] = (unsigned short)(run + incl - c);
                run += lane_of(incl, 63u);
            }
            wave_lds_sync();
#pragma unroll
            for (int u = 0; u < kRankedRounds; ++u)
                if (rel[u] != ~0u) {
                    const uint32_t at = (uint32_t)below[rel[u] >> 5] + (uint32_t)__popc(bm[rel[u] >> 5] & ((1u << (rel[u] & 31u)) - 1u));
                    if (at < cnt_p) hits[w_p + at] = x[u];  // (always: the count is the bisection of this very list)
                }
            wave_lds_sync();  // (the next row clears the bitmap)
        }
    }
}

// What the three fill kernels of the last call served, summed up afterwards from what the call left in its workspace (the
// per-probe arrays and the two work lists) instead of costing every call counters of its own:
//   out[0..5]   rows and entries read of fill_small_kernel, fill_big_kernel, fill_ranked_kernel (the ranked fill reads two
//               entries -- position and slot -- per list position);
//   out[6..17]  rows, sum of R, sum of kept hits of fill_big_kernel's rows with R <= kRankMin, with R above it but counted
//               by streaming, counted by bisection -- and of fill_ranked_kernel's rows (all counted by bisection).
constexpr int kFillAcct = 18;
__global__ __launch_bounds__(256) void fill_account_kernel(RunParams rp, const uint32_t *__restrict__ p_raw,
                                                           const uint32_t *__restrict__ p_filt,
                                                           const uint32_t *__restrict__ big_list,
                                                           const uint32_t *__restrict__ ranked_top,
                                                           unsigned long long *__restrict__ ctr) {
    unsigned long long acc[kFillAcct];
#pragma unroll
    for (int j = 0; j < kFillAcct; ++j) acc[j] = 0;
    const uint32_t n_t = rp.n_tiles(1024u);
    for (uint32_t t = blockIdx.x; t < n_t; t += gridDim.x) {
        uint32_t g_end;
        const uint32_t g0 = rp.tile_of(t, 1024u, g_end);
        for (int a = 0; a < 4; ++a) {
            const uint32_t g = g0 + (uint32_t)a * 256u + threadIdx.x;
            if (g >= g_end) continue;
            const uint32_t f = p_filt[g];
            if (f == 0 || f >= kPending) continue;
            const uint32_t raw = p_raw[g];
            if (raw > (uint32_t)kSmallInterval) continue;
            acc[0] += 1;
            acc[1] += raw;
        }
    }
    const uint64_t n_big = ctr[CT_BIG], n_big0 = ctr[CT_BIG0], n_rk = ctr[CT_RANKED];
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = tid; e < n_big; e += stride) {
        const uint32_t g = big_list[e], f = p_filt[g];
        if (f == 0 || f >= kPending) continue;
        const unsigned long long R = p_raw[g];
        acc[2] += 1;
        acc[3] += R;
        const int cl = e >= n_big0 ? 2 : (R > (unsigned long long)kRankMin ? 1 : 0);
        acc[6 + 3 * cl] += 1;
        acc[7 + 3 * cl] += R;
        acc[8 + 3 * cl] += f;
    }
    for (uint64_t e = tid; e < n_rk; e += stride) {
        const uint32_t g = *(ranked_top - 1 - (long long)e), f = p_filt[g];
        const unsigned long long R = p_raw[g];
        acc[4] += 1;
        acc[5] += 2u * (R > (unsigned long long)f + 1u ? (unsigned long long)f + 1u : R);
        acc[15] += 1;
        acc[16] += R;
        acc[17] += f;
    }
#pragma unroll
    for (int j = 0; j < kFillAcct; ++j) {
        unsigned long long v = acc[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&ctr[CT_FILL_ACCT + j], v);
    }
}

}  // namespace asgart
