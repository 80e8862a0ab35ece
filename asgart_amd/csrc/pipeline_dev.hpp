// pipeline_dev.hpp -- device kernels of the probe -> search -> extend pipeline, up to the extension: the front, the
// placement of the segments onto the extension tiers, the cut planner of the runs over ranges.
//
//   K1 probe_count_kernel   one thread per probe: key, SA interval, filtered count
//   K1b big_count_kernel    one wave per probe with a large interval (early exit)
//   K2 scan_{reduce,mid,down}  row offsets + quiet-run segmentation
//   K3 fill_{small,big}_kernel  filtered hits in SA order -> CSR
// The extension kernels have a file each (extend_{wave,heavy,fast,k8}_dev.hpp) over extend_common_dev.hpp.
//
// Reference semantics: src/automaton.rs:57-216 (see DESIGN.md for the proof
// that a run of ceil(G/step) processed zero-hit probes empties the arm list,
// which is what makes segments independent).
#pragma once

#include "extend_common_dev.hpp"

namespace asgart {

__device__ inline void wave_lds_sync() {  // LDS traffic of ONE wave: what its lanes wrote is there for its other lanes
    __builtin_amdgcn_wave_barrier();
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

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
struct HitRule {
    unsigned long long thr, self;
};
// keep_hit(x, i, s, L, reverse)  ==  x >= thr && x != self
__device__ inline HitRule hit_rule(uint64_t i, uint64_t s, uint64_t L, bool reverse) {
    HitRule h;
    h.thr = reverse ? s + L - i : i + s + 1u;
    h.self = reverse ? i : ~0ull;
    return h;
}
__device__ inline uint32_t lane_get(uint32_t v, uint32_t l) {  // lane l's v, l per lane (every lane takes part)
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(l << 2), (int)v);
}
__device__ inline unsigned long long lane_get(unsigned long long v, uint32_t l) {
    return ((unsigned long long)lane_get((uint32_t)(v >> 32), l) << 32) | lane_get((uint32_t)v, l);
}
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
        const unsigned long long lo_o = lane_get(lo, own), thr_o = lane_get(hr.thr, own), self_o = lane_get(hr.self, own);
        const bool live = e < total;
        SlotT x = 0;
        if (live) x = sa[lo_o + r];
        const bool keep = live && (unsigned long long)x >= thr_o && (unsigned long long)x != self_o;
        round(own, r, x, keep, (unsigned long long)__ballot(keep));
    }
}

// ---------------------------------------------------------------- K1 ---------
// Probe search: one thread per probe, one workgroup per 256 consecutive probes.
//
//   1. The workgroup's probes cover ONE contiguous text window (stride k/2, so 256 probes =
//      2570 bases at k = 20): it is staged into LDS with one coalesced 16-byte load per lane.
//   2. Every base is converted once: thread h packs the 3-bit codes of "half" h (k/2 bases) and
//      the key of probe t is half[t] ++ half[t+1] (plus one more base when k is odd).  -R walks
//      the window downwards, -C complements the codes: needle preparation (reference
//      src/bin/asgart.rs:206-218) without a needle.
//   3. Position bits (RunParams::pbits): one bit per probe, staged with the window; a probe whose
//      bit is clear keeps no hit and is done.
//   4. The others: prefix table -> bisection over the sorted keys -> filtered count of the
//      suffix-array interval (intervals > 32 go to the wave kernel through big_list).
//
// COUNT = true is the accounting pass behind bench.py's `kernel_algorithmic_bytes`: the same
// control flow, no stores, every load / store of the real kernel priced in bytes.
constexpr int kProbeBlock = 256;  // probes per workgroup (one tile)
constexpr int kProbeThreads = 64; // ... run by ONE wave: every lane stages and tests four of them, then the survivors (a tenth of
                                  // the tile on the GRCh38-shaped input since a position bit says "can keep a hit": about 24, on 24
                                  // of the 64 lanes; all 256 while the bits are blank) are looked up.  With four waves per tile
                                  // three of them held their slots through the staging only to retire; a wave slot now spends most
                                  // of its life in the dependent gathers of the lookup, and no barrier involves a second wave.
constexpr int kProbeSub = kProbeBlock / kProbeThreads;
constexpr int kMaxHalf = (kMaxKey + 1) / 2;                                 // bases per half (one-word keys)
constexpr int kWinBytes = ((kProbeBlock + 2) * kMaxHalf + 15 + 16 + 15) / 16 * 16;  // <= 256 lanes x 16 B

template <class SlotT, bool COUNT>
__global__ __launch_bounds__(kProbeThreads) void probe_count_kernel(IndexView<SlotT> ix, RunParams rp,
                                                                    SlotT *__restrict__ p_lo,
                                                                    uint32_t *__restrict__ p_raw,
                                                                    uint32_t *__restrict__ p_filt,
                                                                    uint32_t *__restrict__ big_list,
                                                                    uint32_t *__restrict__ rank_list,
                                                                    unsigned long long *__restrict__ ctr) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[kWinBytes];
    __shared__ uint32_t s_half[kProbeBlock + 2];
    // the position bits of the workgroup's probes: 256 probes at stride k/2 = one contiguous run of bits
    constexpr int kPbLoads = (kProbeBlock * kMaxHalf + 127) / 128 + 2;  // 16-byte loads that cover it
    __shared__ __attribute__((aligned(16))) uint32_t s_pb[kPbLoads * 4];
    __shared__ uint8_t s_surv[kProbeBlock];
    typename std::conditional<COUNT, CountBytes, NoBytes>::type cb;
    const uint32_t lane = threadIdx.x;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    uint32_t g_end;  // end of the tile's window
    const uint32_t gb = rp.tile_of(blockIdx.x, (uint32_t)kProbeBlock, g_end);  // first probe of the workgroup
    const uint32_t g_last = min(gb + (uint32_t)kProbeBlock, g_end) - 1u;
    const int k = rp.k, H = rp.step;
    // one chunk for the whole workgroup (all but a handful of workgroups): staged window
    const int c0 = chunk_of_uniform(rp.ch, gb);
    // (probes longer than one key word -- rare -- take the per-thread path as well)
    const bool uniform = rp.ch.pbase[c0 + 1] > g_last && k <= kMaxKey;
    uint32_t n_rej = 0;
    // one probe's lookup: SA interval, filtered count of a small interval (large ones are marked for the wave kernels)
    // lrn_: the pass's position bits (RunParams::pbits), or null
    auto lookup = [&](uint32_t g_, uint64_t q_, uint64_t q2_, uint64_t i_, uint64_t s_, uint64_t L_, uint32_t md_,
                      const uint64_t *lrn_) {
        const bool reverse = (md_ & 2u) != 0u, complement = (md_ & 1u) != 0u;
        uint64_t lo, hi;
        ProbeRef pr;  // (read only by probes of more than 42 bases)
        pr.p = reverse ? ix.text + s_ + L_ - 1u - i_ : ix.text + s_ + i_;
        pr.dir = reverse ? -1 : 1;
        pr.comp = complement;
        const bool all_occurrences = kmer_range(ix, q_, q2_, pr, lo, hi, cb);
        const uint64_t raw = hi - lo;
        if (!COUNT) {
            p_lo[g_] = (SlotT)lo;
            p_raw[g_] = (uint32_t)raw;
        }
        cb.wr(sizeof(SlotT) + 4);
        if (raw <= (uint64_t)kSmallInterval) {
            uint32_t cnt = 0;
            // Direct pass: the needle is the text itself, so the probe's own position is one of
            // the occurrences; a single occurrence is that one, and the filter (x > i + s)
            // drops it -- no need to fetch the suffix-array entry.
            const bool only_self = all_occurrences && raw == 1 && md_ == 0u;
            bool any = false;  // an occurrence that could be kept, whatever chunk the probe came in (a reversed needle's
                               // `m.start != i` compares a text position with a chunk offset: left out)
            for (uint64_t r = lo; r < hi && !only_self; ++r) {
                cb.rd(sizeof(SlotT));
                const uint64_t x = ix.sa[r];
                cnt += keep_hit(x, i_, s_, L_, reverse) ? 1u : 0u;
                if (reverse) any |= x >= s_ + L_ - i_;
            }
            if (!reverse) any = cnt != 0u;
            if (!COUNT) p_filt[g_] = cnt > rp.C ? kSkipCard : cnt;
            cb.wr(4);
            if constexpr (!COUNT) {
                // learned position bits: no occurrence of this probe's k-mer can ever be kept at this text position
                if (lrn_ && all_occurrences && !any) {
                    const uint64_t p = reverse ? s_ + L_ - i_ - (uint64_t)k : s_ + i_;
                    atomicAnd(const_cast<unsigned long long *>(reinterpret_cast<const unsigned long long *>(lrn_)) + (p >> 6),
                              ~(1ull << (p & 63u)));
                }
            }
        } else {
            // a large interval is only MARKED here; collect_pending_kernel turns the marks into the two work lists (a
            // workgroup-aggregated append from this kernel cost every workgroup a returning atomic on one of two adjacent
            // counters and a barrier that its retired waves never reached).
            // a whole k-mer interval of some size: its kept count is a bisection of the position-sorted list
            if (!COUNT) p_filt[g_] = (ix.sap && all_occurrences && raw > (uint64_t)kRankMin) ? kPendingRank : kPending;
            cb.wr(4 + 4);  // + its work-list entry (written by the collecting pass)
            cb.rd(4);      //   ... which reads the mark back
        }
    };
    // a probe the position bits (or its first base) answer: what is written for it; -> true: it has to be looked up
    auto screen = [&](uint32_t g_, uint32_t first_, bool pass_, uint32_t md_) {
        if (first_ == 4u) {  // needle[i] == 'N'  (automaton.rs:100-102)
            if (!COUNT) p_filt[g_] = kSkipN;
            cb.wr(4);
            return false;
        }
        if (!pass_) {
            // the position filter says: no hit is kept (the probe's interval is never looked up; asgart_get_stats does that
            // when the raw interval sizes are asked for)
            if (!COUNT) {
                p_raw[g_] = kRawUnknown;
                p_filt[g_] = 0u;
            }
            cb.wr(8);
            n_rej += 1;
            return false;
        }
        return true;
    };
    if (uniform) {
        const uint32_t pass0 = rp.pass_of(c0), md = rp.mode_of_pass(pass0);  // (the orientation of the chunk's pass)
        const bool reverse = (md & 2u) != 0u, complement = (md & 1u) != 0u;
        const uint64_t *const pbits = rp.pbits[pass0];
        const uint64_t s = rp.ch.start[c0], L = rp.ch.len[c0];
        const uint64_t i0 = (uint64_t)(gb - rp.ch.pbase[c0] + 1) * (uint64_t)H;  // needle offset of probe gb
        const int n_half = kProbeBlock + 2;
        // text positions of half h, base j:  direct  b0 + h*H + j ;  reversed  e0 - h*H - j
        const long long b0 = (long long)(s + i0), e0 = (long long)(s + L - 1u - i0);
        const long long w_lo = reverse ? e0 - (long long)n_half * H + 1 : b0;
        const long long a_lo = w_lo & ~15ll;  // floor to 16 (two's complement: also for negatives)
        const long long w_hi = reverse ? e0 : b0 + (long long)n_half * H - 1;  // inclusive
        const uint32_t n_load = (uint32_t)((w_hi - a_lo) / 16 + 1);  // <= kWinBytes / 16
        for (uint32_t t = lane; t < n_load; t += kProbeThreads) {   // (three rounds, all in flight together)
            const long long a = a_lo + 16ll * t;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (a >= 0 && (uint64_t)a + 16u <= ix.n + 64u) {  // the text allocation has 64 spare bytes
                v = *reinterpret_cast<const uint4 *>(ix.text + a);
                cb.rd16();
            }
            *reinterpret_cast<uint4 *>(s_text + 16u * t) = v;
        }
        long long pb_lo = 0;  // first bit held by s_pb
        if (pbits) {
            // text positions the probes cover: direct  s + i0 + t H ;  reversed  s + L - i0 - k - t H
            const long long p_first = reverse ? (long long)(s + L - i0) - k - (long long)(kProbeBlock - 1) * H
                                                 : (long long)(s + i0);
            const long long byte_lo = (p_first >> 7) * 16;  // (floor: also for the negatives of the idle lanes)
            pb_lo = byte_lo * 8;
            const long long p_last = p_first + (long long)(kProbeBlock - 1) * H;
            const uint32_t n_pb = (uint32_t)((p_last >> 7) - (p_first >> 7) + 1);  // <= kPbLoads
            if (lane < n_pb) {
                const long long a = byte_lo + 16ll * lane;
                uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
                if (a >= 0 && (uint64_t)a + 16u <= ((ix.n + 63u) / 64u) * 8u + 512u) {  // (the allocation is padded)
                    v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(pbits) + a);
                    cb.rd16();
                }
                *reinterpret_cast<uint4 *>(&s_pb[4u * lane]) = v;
            }
        }
        __syncthreads();  // (one wave: the barrier orders its own LDS traffic)
        for (uint32_t h = lane; h < (uint32_t)n_half; h += kProbeThreads) {
            const long long p0 = reverse ? (e0 - a_lo) - (long long)h * H : (b0 - a_lo) + (long long)h * H;
            uint32_t v = 0;
            for (int j = 0; j < H; ++j) {
                uint32_t c = base_code(s_text[reverse ? p0 - j : p0 + j]);
                if (complement) c = comp_code(c);
                v = (v << 3) | c;
            }
            s_half[h] = v;
        }
        __syncthreads();
        auto key_of = [&](uint32_t t) {
            uint64_t qt = ((uint64_t)s_half[t] << (3 * H)) | (uint64_t)s_half[t + 1];
            if (k & 1) qt = (qt << 3) | (uint64_t)(s_half[t + 2] >> (3 * (H - 1)));
            return qt;
        };
        // ---- position bits (every probe), then the lookup of the survivors ---------------------------------
        // About nine probes in ten are answered by the bits.  The lookup behind it -- prefix table, key bisection,
        // suffix-array entries -- is a chain of dependent random gathers, and a wave runs it at the speed of its
        // slowest lane however few lanes are left: the survivors of the tile are compacted (ballots) so that the
        // lookups run on the lowest lanes, 64 survivors at a time.
        uint32_t n_surv = 0;
#pragma unroll
        for (int u = 0; u < kProbeSub; ++u) {
            const uint32_t t = lane + (uint32_t)u * kProbeThreads, g = gb + t;
            bool survivor = false;
            if (g < g_end) {
                const uint64_t q = key_of(t);
                const uint32_t first = (uint32_t)(q >> (3 * (k - 1))) & 7u;
                bool pass = true;
                if (first != 4u) {
                    const uint64_t i = i0 + (uint64_t)t * (uint64_t)H;
                    if (pbits) {  // the bit of the text position the probe covers
                        const long long p = reverse ? (long long)(s + L - i) - k : (long long)(s + i);
                        const uint32_t b = (uint32_t)(p - pb_lo);
                        pass = (s_pb[b >> 5] >> (b & 31u)) & 1u;
                    }
                }
                survivor = screen(g, first, pass, md);
            }
            const unsigned long long sm = __ballot(survivor);
            if (survivor) s_surv[n_surv + (uint32_t)__popcll(sm & lt_mask)] = (uint8_t)t;
            n_surv += (uint32_t)__popcll(sm);
        }
        __syncthreads();
        for (uint32_t j = lane; j < n_surv; j += kProbeThreads) {
            const uint32_t t = s_surv[j];
            lookup(gb + t, key_of(t), 0ull, i0 + (uint64_t)t * (uint64_t)H, s, L, md, pbits);
        }
    } else {
        // the tile straddles a chunk boundary (or the probes are longer than one key word): every probe on its own
#pragma unroll 1
        for (int u = 0; u < kProbeSub; ++u) {
            const uint32_t g = gb + lane + (uint32_t)u * kProbeThreads;
            if (g >= g_end) continue;
            const int c = chunk_of(rp.ch, g);
            const uint32_t pass_c = rp.pass_of(c), md = rp.mode_of_pass(pass_c);
            const bool reverse = (md & 2u) != 0u, complement = (md & 1u) != 0u;
            const uint64_t *const pbits = rp.pbits[pass_c];
            const uint64_t s = rp.ch.start[c], L = rp.ch.len[c];
            const uint64_t i = (uint64_t)(g - rp.ch.pbase[c] + 1) * (uint64_t)H;
            uint32_t first = 0;
            uint64_t q2 = 0;
            const uint64_t q = probe_key(ix.text, s, L, i, k, reverse, complement, &first, &q2);
            cb.rd((uint32_t)k);
            bool pass = true;
            if (first != 4u && pbits) {
                const long long p = reverse ? (long long)(s + L - i) - k : (long long)(s + i);
                cb.rd(8);
                pass = (pbits[(uint64_t)p >> 6] >> ((uint64_t)p & 63u)) & 1ull;
            }
            if (screen(g, first, pass, md)) lookup(g, q, q2, i, s, L, md, pbits);
        }
    }
    if constexpr (COUNT) {
        unsigned long long b = cb.n, r = n_rej, b16 = cb.n16;
        for (int off = 32; off > 0; off >>= 1) {
            b += __shfl_down(b, off);
            r += __shfl_down(r, off);
            b16 += __shfl_down(b16, off);
        }
        if (lane == 0) {
            atomicAdd(&ctr[CT_ALG_BYTES], b);
            if (r) atomicAdd(&ctr[CT_FLT_REJECTED], r);
            if (b16) atomicAdd(&ctr[CT_ALG_BYTES16], b16);
        }
    }
}

// The probes probe_count_kernel marked as large intervals -> the two work lists (big_list: counted by streaming the
// interval; rank_list: by bisection of its position-sorted list).  Persistent workgroups over contiguous spans of the
// probe sequence: the marks of a tile are compacted by wave ballots into two LDS buffers, which are appended to the
// lists with ONE global atomic per 2 K entries instead of one (or two) per 256 probes.  Streams 4 bytes per probe.
constexpr int kCollectBlock = 256, kCollectItems = 8, kCollectTile = kCollectBlock * kCollectItems;
constexpr int kCollectCap = 2 * kCollectTile;
__global__ __launch_bounds__(kCollectBlock) void collect_pending_kernel(RunParams rp, const uint32_t *__restrict__ p_filt,
                                                                        uint32_t *__restrict__ big_list,
                                                                        uint32_t *__restrict__ rank_list,
                                                                        unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t s_buf[2][kCollectCap];
    __shared__ uint32_t s_cnt[2];
    __shared__ unsigned long long s_base[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t n_tiles = rp.n_tiles((uint32_t)kCollectTile);
    // a contiguous run of tiles per workgroup (the lists then follow the probe order in long stretches)
    const uint32_t t0 = (uint32_t)((uint64_t)n_tiles * blockIdx.x / gridDim.x);
    const uint32_t t1 = (uint32_t)((uint64_t)n_tiles * (blockIdx.x + 1u) / gridDim.x);
    auto flush = [&](int which, uint32_t *__restrict__ list, int counter) {  // (workgroup-uniform)
        const uint32_t n = s_cnt[which];
        if (!n) return;
        if (tid == 0) s_base[which] = atomicAdd(&ctr[counter], (unsigned long long)n);
        __syncthreads();
        const unsigned long long b = s_base[which];
        for (uint32_t j = tid; j < n; j += kCollectBlock) list[b + j] = s_buf[which][j];
        __syncthreads();
        if (tid == 0) s_cnt[which] = 0;
        __syncthreads();
    };
    for (uint32_t t = t0; t < t1; ++t) {
        uint32_t g_end;
        const uint32_t g0 = rp.tile_of(t, (uint32_t)kCollectTile, g_end);
#pragma unroll
        for (int a = 0; a < kCollectItems; ++a) {
            const uint32_t g = g0 + (uint32_t)a * kCollectBlock + tid;  // coalesced
            const uint32_t f = g < g_end ? p_filt[g] : 0u;
            const bool big = f == kPending, rank = f == kPendingRank;
            const unsigned long long mb = __ballot(big), mr = __ballot(rank);
            if (mb) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&s_cnt[0], (uint32_t)__popcll(mb));
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (big) s_buf[0][base + (uint32_t)__popcll(mb & lt_mask)] = g;
            }
            if (mr) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&s_cnt[1], (uint32_t)__popcll(mr));
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (rank) s_buf[1][base + (uint32_t)__popcll(mr & lt_mask)] = g;
            }
        }
        __syncthreads();
        // (the decision is taken from a snapshot every thread has read BEFORE anyone may add the next tile's entries:
        // a wave that ran ahead into the next tile's atomics could otherwise push a slower wave's reading over the
        // threshold and send only that wave into flush() and its barriers)
        const uint32_t c0 = s_cnt[0], c1 = s_cnt[1];
        __syncthreads();
        if (c0 > (uint32_t)(kCollectCap - kCollectTile)) flush(0, big_list, CT_BIG);
        if (c1 > (uint32_t)(kCollectCap - kCollectTile)) flush(1, rank_list, CT_RANK);
    }
    flush(0, big_list, CT_BIG);
    flush(1, rank_list, CT_RANK);
}

// Large whole-k-mer intervals when the index holds the position-sorted occurrence lists: the hit filter keeps the
// occurrences beyond a position threshold (src/automaton.rs:105-114), so the kept count is one bisection of
// sap[lo..hi) -- a dozen gathers instead of the ~1000 suffix-array entries a probe of a frequent k-mer streams
// before the early exit at max_cardinality + 1.  One thread per interval.  Probes that stay below the cardinality
// limit are appended to big_list, from which fill_big_kernel materialises their hits (in suffix-array order) -- or, where
// the kept tail of the list is much shorter than the interval (ranked_fill_takes), to the ranked list, which grows from
// ranked_top downwards (the END of big_list's buffer: no probe is in both) and is served by fill_ranked_kernel.
template <class SlotT, bool COUNT>
__global__ __launch_bounds__(256) void rank_count_kernel(IndexView<SlotT> ix, RunParams rp,
                                                         const SlotT *__restrict__ p_lo,
                                                         const uint32_t *__restrict__ p_raw,
                                                         uint32_t *__restrict__ p_filt,
                                                         const uint32_t *__restrict__ rank_list,
                                                         uint32_t *__restrict__ big_list,
                                                         uint32_t *__restrict__ ranked_top, int ranked_mode,
                                                         unsigned long long *__restrict__ ctr) {
    const uint64_t n_rank = ctr[CT_RANK];
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long bytes = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63ull; e0 < n_rank; e0 += stride) {
        const uint64_t e = e0 + lane;
        bool refill = false, ranked = false;
        uint32_t g = 0;
        if (e < n_rank) {
            g = rank_list[e];
            const int c = chunk_of(rp.ch, g);
            const uint64_t s = rp.ch.start[c], L = rp.ch.len[c];
            const uint64_t i = (uint64_t)(g - rp.ch.pbase[c] + 1) * (uint64_t)rp.step;
            const SlotT *__restrict__ a = ix.sap + p_lo[g];
            const uint64_t R = p_raw[g];
            bytes += 4 + sizeof(SlotT) + 4 + 4;  // list entry, interval, final count
            // first index whose position is >= t
            auto first_ge = [&](uint64_t t) {
                uint64_t lo = 0, hi = R;
                while (lo < hi) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    bytes += sizeof(SlotT);
                    if ((uint64_t)a[mid] < t) lo = mid + 1; else hi = mid;
                }
                return lo;
            };
            uint64_t cnt;
            if (!(rp.mode_of(c) & 2u)) {
                cnt = R - first_ge(i + s + 1u);  // keep_hit: x > i + s
            } else {
                const uint64_t t = s + L - i;  // keep_hit: x != i && x >= s + L - i
                cnt = R - first_ge(t);
                if (i >= t) {
                    const uint64_t j = first_ge(i);
                    if (j < R && (uint64_t)a[j] == i) --cnt;
                }
            }
            const uint32_t f = cnt > (uint64_t)rp.C ? kSkipCard : (uint32_t)cnt;
            if (!COUNT) p_filt[g] = f;
            refill = f != 0u && f < kPending;
            ranked = refill && ranked_fill_takes(R, cnt, ranked_mode);
        }
        if (!COUNT) {
            const unsigned long long lt = (1ull << lane) - 1ull;
            const unsigned long long m = __ballot(refill && !ranked), mr = __ballot(ranked);
            if (m) {
                const int leader = __ffsll((long long)m) - 1;
                unsigned long long at = 0;
                if ((int)lane == leader) at = atomicAdd(&ctr[CT_BIG], (unsigned long long)__popcll(m));
                at = __shfl(at, leader);
                if (refill && !ranked) big_list[at + __popcll(m & lt)] = g;
            }
            if (mr) {
                const int leader = __ffsll((long long)mr) - 1;
                unsigned long long at = 0;
                if ((int)lane == leader) at = atomicAdd(&ctr[CT_RANKED], (unsigned long long)__popcll(mr));
                at = __shfl(at, leader);
                if (ranked) *(ranked_top - 1 - (long long)(at + __popcll(mr & lt))) = g;
            }
        } else {
            bytes += refill ? 4u : 0u;
        }
    }
    if (COUNT) {
        for (int off = 32; off > 0; off >>= 1) bytes += __shfl_down(bytes, off);
        if (lane == 0 && bytes) atomicAdd(&ctr[CT_ALG_BYTES], bytes);
    }
}

// Large intervals, one wave per 64 of them: the per-probe set-up (work-list entry, chunk, interval) is a
// chain of dependent global loads, so the 64 lanes each set up one probe at the same time; the wave then
// counts the intervals one after the other -- 256 suffix-array entries per round trip, early exit at
// max_cardinality + 1 -- with the first round of the NEXT interval already in flight.
template <class SlotT, bool COUNT>
__global__ __launch_bounds__(256) void big_count_kernel(IndexView<SlotT> ix, RunParams rp,
                                                        const SlotT *__restrict__ p_lo,
                                                        const uint32_t *__restrict__ p_raw,
                                                        uint32_t *__restrict__ p_filt,
                                                        const uint32_t *__restrict__ big_list,
                                                        unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    // (the accounting pass runs after the call: the list has grown by what rank_count_kernel appended for the fill)
    const uint64_t n_big = COUNT ? ctr[CT_BIG0] : ctr[CT_BIG];
    if (!COUNT && blockIdx.x == 0 && threadIdx.x == 0) ctr[CT_BIG0] = n_big;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long bytes = 0;
    for (uint64_t e0 = wave * 64u; e0 < n_big; e0 += n_waves * 64u) {
        const uint32_t np = (uint32_t)min((uint64_t)64, n_big - e0);
        // lane l sets up probe e0 + l
        uint32_t g = 0, md = 0;
        unsigned long long s = 0, L = 0, i = 0, lo = 0, hi = 0;
        if (lane < np) {
            g = big_list[e0 + lane];
            const int c = chunk_of(rp.ch, g);
            md = rp.mode_of(c);
            s = rp.ch.start[c];
            L = rp.ch.len[c];
            i = (unsigned long long)(g - rp.ch.pbase[c] + 1) * (unsigned long long)rp.step;
            lo = p_lo[g];
            hi = lo + p_raw[g];
        }
        bytes += (unsigned long long)np * (4 + sizeof(SlotT) + 4 + 4);  // list entry, interval, final count
        uint32_t my_cnt = 0;
        // first round of probe 0
        SlotT xn[4];
        {
            const unsigned long long l0 = lane_of(lo, 0u), h0 = lane_of(hi, 0u);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned long long r = l0 + 64u * u + lane;
                xn[u] = r < h0 ? ix.sa[r] : (SlotT)0;
            }
        }
        for (uint32_t p = 0; p < np; ++p) {
            const unsigned long long lo_p = lane_of(lo, p), hi_p = lane_of(hi, p), i_p = lane_of(i, p),
                                     s_p = lane_of(s, p), L_p = lane_of(L, p);
            const bool rev_p = (lane_of(md, p) & 2u) != 0u;
            SlotT x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = xn[u];
            if (p + 1 < np) {  // the next interval's first 256 entries: in flight while this one is counted
                const unsigned long long l1 = lane_of(lo, p + 1u), h1 = lane_of(hi, p + 1u);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned long long r = l1 + 64u * u + lane;
                    xn[u] = r < h1 ? ix.sa[r] : (SlotT)0;
                }
            }
            unsigned long long cnt = 0;
            for (unsigned long long base = lo_p;;) {
                bytes += sizeof(SlotT) * (hi_p - base < 256u ? hi_p - base : 256u);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned long long r = base + 64u * u + lane;
                    const bool keep = r < hi_p && keep_hit(x[u], i_p, s_p, L_p, rev_p);
                    cnt += __popcll(__ballot(keep));
                }
                base += 256;
                if (base >= hi_p || cnt > rp.C) break;
#pragma unroll
                for (int u = 0; u < 4; ++u) {  // (the early exit makes the rounds dependent; requesting the next
                                               // round ahead of the count was measured: 7.0 -> 8.2 ms, more bytes)
                    const unsigned long long r = base + 64u * u + lane;
                    x[u] = r < hi_p ? ix.sa[r] : (SlotT)0;
                }
            }
            if (lane == p) my_cnt = cnt > rp.C ? kSkipCard : (uint32_t)cnt;
        }
        if (!COUNT && lane < np) p_filt[g] = my_cnt;
    }
    if (COUNT && lane == 0 && bytes) atomicAdd(&ctr[CT_ALG_BYTES], bytes);
}

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

// The sum of the raw interval sizes over the searched probes (asgart_stats.raw_hits: a statistic of the call, wanted by
// the parity tests and the bench's yardstick, not by the path) -- computed when the statistics are asked for, from the
// per-probe arrays the call left in its workspace, instead of costing every call a second read of 4 bytes per probe.
// A probe the position filter answered has no interval there (p_raw = kRawUnknown): its k-mer is looked up here.
template <class SlotT>
__global__ __launch_bounds__(256) void raw_hits_kernel(IndexView<SlotT> ix, RunParams rp, const uint32_t *__restrict__ p_filt,
                                                       const uint32_t *__restrict__ p_raw, unsigned long long *__restrict__ out) {
    unsigned long long sum = 0;
    const uint32_t n_t = rp.n_tiles(1024u);
    for (uint32_t t = blockIdx.x; t < n_t; t += gridDim.x) {
        uint32_t g_end;
        const uint32_t g0 = rp.tile_of(t, 1024u, g_end);
#pragma unroll 1
        for (int a = 0; a < 4; ++a) {
            const uint32_t g = g0 + (uint32_t)a * 256u + threadIdx.x;
            if (g >= g_end || p_filt[g] == kSkipN) continue;
            uint32_t raw = p_raw[g];
            if (raw == kRawUnknown) {
                const int c = chunk_of(rp.ch, g);
                const uint32_t md = rp.mode_of(c);
                const uint64_t cs = rp.ch.start[c], cl = rp.ch.len[c];
                const uint64_t i = (uint64_t)(g - rp.ch.pbase[c] + 1) * (uint64_t)rp.step;
                uint32_t first = 0;
                uint64_t q2 = 0, lo, hi;
                const uint64_t q = probe_key(ix.text, cs, cl, i, rp.k, (md & 2u) != 0u, (md & 1u) != 0u, &first, &q2);
                ProbeRef pr;
                pr.p = (md & 2u) ? ix.text + cs + cl - 1u - i : ix.text + cs + i;
                pr.dir = (md & 2u) ? -1 : 1;
                pr.comp = (md & 1u) != 0u;
                kmer_range(ix, q, q2, pr, lo, hi);
                raw = (uint32_t)(hi - lo);
            }
            sum += raw;
        }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(out, sum);
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
            hr = hit_rule((uint64_t)(g - rp.ch.pbase[c] + 1) * (uint64_t)rp.step, rp.ch.start[c], rp.ch.len[c],
                          (rp.mode_of(c) & 2u) != 0u);
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
        unsigned long long s = 0, L = 0, i = 0, lo = 0, hi = 0, w0 = 0;
        uint32_t md = 0;
        bool want = false;
        if (lane < np) {
            const uint32_t g = big_list[e0 + lane];
            const uint32_t f = p_filt[g];
            want = f != 0 && f < kPending;  // skipped / empty rows have nothing to fill
            if (want) {
                const int c = chunk_of(rp.ch, g);
                md = rp.mode_of(c);
                s = rp.ch.start[c];
                L = rp.ch.len[c];
                i = (unsigned long long)(g - rp.ch.pbase[c] + 1) * (unsigned long long)rp.step;
                lo = p_lo[g];
                hi = lo + p_raw[g];
                w0 = row_off[g];
            }
        }
        unsigned long long todo = __ballot(want);
        while (todo) {
            const uint32_t p = (uint32_t)(__ffsll((long long)todo) - 1);
            todo &= todo - 1;
            const unsigned long long lo_p = lane_of(lo, p), hi_p = lane_of(hi, p), i_p = lane_of(i, p),
                                     s_p = lane_of(s, p), L_p = lane_of(L, p);
            const bool rev_p = (lane_of(md, p) & 2u) != 0u;
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
                    const bool keep = r < hi_p && keep_hit(x[u], i_p, s_p, L_p, rev_p);
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
        unsigned long long s = 0, L = 0, i = 0, lo = 0, a0 = 0, w0 = 0;
        uint32_t md = 0, cnt = 0, R = 0;
        if (lane < np) {
            const uint32_t g = *(ranked_top - 1 - (long long)(e0 + lane));
            cnt = min(p_filt[g], (uint32_t)kRankedCap);              // (1..kRankedCap: ranked_fill_takes)
            R = min(p_raw[g], (uint32_t)kRankedMaxR);                // (<= kRankedMaxR: likewise)
            const int c = chunk_of(rp.ch, g);
            md = rp.mode_of(c);
            s = rp.ch.start[c];
            L = rp.ch.len[c];
            i = (unsigned long long)(g - rp.ch.pbase[c] + 1) * (unsigned long long)rp.step;
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
            const unsigned long long lo_p = lane_of(lo, p), a0_p = lane_of(a0, p), i_p = lane_of(i, p), s_p = lane_of(s, p),
                                     L_p = lane_of(L, p), w_p = lane_of(w0, p);
            const bool rev_p = (lane_of(md, p) & 2u) != 0u;
            const uint32_t cnt_p = lane_of(cnt, p), R_p = lane_of(R, p);
            const unsigned long long a1_p = lo_p + R_p;
            SlotT x[kRankedRounds];
            uint32_t rel[kRankedRounds];  // slot inside the interval; ~0u: not kept
#pragma unroll
            for (int u = 0; u < kRankedRounds; ++u) {
                const unsigned long long r = a0_p + 64u * u + lane;
                x[u] = xn[u];
                const uint32_t d = (uint32_t)sn[u] - (uint32_t)lo_p;
                rel[u] = r < a1_p && keep_hit(x[u], i_p, s_p, L_p, rev_p) && d < R_p ? d : ~0u;
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

// ---------------------------------------------------------------- placement ---
// Every live arm was created or extended by a distinct hit of the last t* processed probes, so
// B = max over probes of (hits of this probe + hits of the previous t* processed probes) bounds
// live arms + new arms from above: the tier whose capacity fits B never overflows (the cascade
// serves the tiers that accept segments above their capacity by an allowance, and the test knobs).
// key = (tier-1) << 29 | (2^29-1 - min(total hits, 2^29-1)): ascending sort = tier, longest first.
struct PlaceParams {
    uint32_t cap[kTiers - 1];   // live-arm capacity of tiers 1..kTiers-1 (0: tier unused); the last takes the rest
    uint32_t sum1;              // segments with more hits than this never go to the one-wave tier
    int force_tier;             // tests: minimum tier for segments with a multi-hit probe
    uint32_t long3;             // > 0: tier 3 is reserved for segments of at least this many probes
    uint32_t long3_big;         // ... or this many, for segments beyond tier 5's capacity
    uint32_t dense6;            // > 0: segments bound for tier 6 by their arms go to tier 3 (when they fit it) with at least this
                                // many hits per processed probe: the dense ones of ANY length on the kernel with a control wave
    uint32_t stats;             // 1 (option debug): hit-probes and hits per tier are tallied (one atomic pair per segment)
    uint32_t barren;            // 1: segments that provably emit nothing are not run at all (segment_is_barren)
    uint2 *seg_info;            // per segment, for cluster_barren_kernel: x = hits, y = probe positions walked | bit 31: the walk saw the
                                // segment's end (not cut short by a sharded call's window); null: not recorded
    uint32_t k, step, G;        // (of the call: for that bound)
    unsigned long long M;
    uint32_t dense3;            // > 0: ... and only the DENSE ones (at least this many hits per processed probe on average:
                                // tandem arrays); the sparse long ones (a chromosome against its homologue: a few hits per
                                // probe, mostly run by one wave alone) go to tier 6's kernel -- set when tier 3 runs the
                                // kernel with a control wave, whose step costs the same whatever the probe holds
    uint32_t tail_hits[kTiers - 1];  // tail_hits[t - 1] > 0 (tiers 2, 4, 5): a segment its arm bound sends to tier t goes, with at least this
                                // many hits, to the next tier that holds more instead (the tail rule, place_tier); 0: tier t keeps its own
};

// A segment that cannot emit anything need not run.  A family holds the arms whose RIGHT segment is at least M long
// (src/automaton.rs:186-196), and a right segment only grows when its arm is extended (:136-143): to m.end = x + k with
// x < right.end + threshold (:68-70), i.e. by at most threshold + k - 1 per extension, at most once per hit-probe.  With
// H hit-probes in the segment an arm born at the first is extended at most H - 1 times, and its threshold
// max(G, len(left) / 10) is at most max(G, (span * step + k) / 10) while the segment spans `span` probe positions
// (len(left) = i + k - left.start <= span * step + k).  So
//     k + (H - 1) * (thr_max + k - 1) < M   =>   no arm of the segment ever reaches M: it emits no family, and -- segments being
// independent automaton instances -- leaving it out changes nothing.  At the defaults (k = 20, G = 120,
// M = 1000) that is every segment of up to 8 hit-probes: most of the million-odd tiny segments of a genome-sized pass.
// (Not when the walk was cut short by the end of a sharded call's window: the segment may go on beyond it.)
constexpr int kTierBarren = kTiers + 1;
__device__ inline bool segment_is_barren(const PlaceParams &pp, uint32_t n_hit, uint32_t span_probes) {
    if (!pp.barren || n_hit == 0u) return false;
    const unsigned long long len_left_max = (unsigned long long)span_probes * pp.step + pp.k;
    const unsigned long long thr_max = max((unsigned long long)pp.G, len_left_max / 10ull);
    return (unsigned long long)pp.k + (unsigned long long)(n_hit - 1u) * (thr_max + pp.k - 1ull) < pp.M;
}

// Sort key of a segment inside its tier (ascending = launch order).  Heavy tiers: longest first,
// so that the serial chains start early.  Tier 1 holds over a million mostly tiny segments whose
// cost is the latency of fetching their probe rows: apart from its few long ones (first, by
// length) they run in genome order, so that the segments in flight at any time share cache lines
// and pages of p_filt / row_off / hits.
__device__ inline uint32_t placement_key(int tier, unsigned long long sum, uint32_t g0) {
    uint32_t low;
    if (tier == 1) {
        low = sum >= 1024ull ? 1023u - (uint32_t)min(sum >> 5, 1023ull) : 1024u + (g0 >> 4);
    } else {
        const uint32_t s29 = sum > 0x1FFFFFFFull ? 0x1FFFFFFFu : (uint32_t)sum;
        low = 0x1FFFFFFFu - s29;
    }
    return (((uint32_t)tier - 1u) << 29) | low;
}

// The next tier above src that is in use and holds more arms than src (cap[t - 1]: tier t's capacity, 0: not in use; tier
// kTiers takes whatever is left); tier `skip` is passed over.  Where the cascade re-runs what src gave up on (skip = 0), and
// where the tail rule sends a long segment (skip = 3).
__host__ __device__ inline int next_holding_more(const uint32_t *cap, int src, int skip = 0) {
    int dst = src + 1;
    while (dst < kTiers && (dst == skip || cap[dst - 1] == 0u || cap[dst - 1] <= cap[src - 1])) ++dst;
    return dst;
}

// Tier of a segment from its live-arm bound, hit total and processed-probe count.  With long3 set,
// tier 3 (lowest per-probe latency, one workgroup of 1024 threads per CU) only takes the long
// segments whose serial chain is the critical path of a pass; everything else goes by capacity.
// The tail rule: a launch lasts as long as its longest segment, and a stream that carries two launches (a call has fewer
// hardware queues than tiers) runs the second one's longest segment behind the first one's.  The few segments that make up
// the tail of a thresholded tier -- those with tail_hits hits and more -- go to the next arm-resident workgroup tier (4, 5,
// 6) that holds more, whose launch a longer segment bounds anyway.  More capacity is always safe; tier 3 is never entered
// this way (long3 / dense3 / dense6 decide that, above and below).  *tail_up: the rule moved the segment.
__device__ inline int place_tier(uint32_t bound, unsigned long long sum, uint32_t n_probes, const PlaceParams &pp, bool *tail_up) {
    *tail_up = false;
    if (bound <= pp.cap[0] && sum <= pp.sum1) return 1;
    // tier 6 pays ~3x tier 3's time per probe (many arms per thread): its segments count as long
    // from a quarter of the threshold on
    if (pp.long3 && bound <= pp.cap[2] &&
        (n_probes >= pp.long3 || (bound > pp.cap[4] && n_probes >= pp.long3_big))) {
        if (!pp.dense3 || sum >= (unsigned long long)pp.dense3 * n_probes || bound > pp.cap[5]) return 3;
        return 6;  // (the long segments that are not dense: mostly run by one wave alone, on K6's solo probes)
    }
    for (int t = 2; t < kTiers; ++t) {
        if (t == 3 && pp.long3) continue;
        if (bound <= pp.cap[t - 1]) {
            if (t == 6 && pp.dense6 && bound <= pp.cap[2] && sum >= (unsigned long long)pp.dense6 * n_probes) return 3;
            if (pp.tail_hits[t - 1] && sum >= (unsigned long long)pp.tail_hits[t - 1]) {
                const int up = next_holding_more(pp.cap, t, 3);
                if (up >= 4 && up <= 6) {
                    *tail_up = true;
                    return up;
                }
            }
            return t;
        }
    }
    return kTiers;
}

// The placement walk reads the per-probe hit counts only -- no hit accesses at all.
//
// Most segments are a handful of probes long (3.4 M segments per GRCh38-shaped step, a dozen probes each), and a
// wave per segment spends its time on the per-segment chain of dependent loads.  So the first kernel walks ONE
// SEGMENT PER LANE, 64 segments per wave side by side, for at most kLaneWalk probes; the few segments that are
// longer go to a list and the wave-per-segment kernel below (64 probes per round trip) finishes them.
constexpr uint32_t kLaneWalk = 256;

__global__ __launch_bounds__(64) void seg_stats_lanes_kernel(RunParams rp, const uint32_t *__restrict__ p_filt,
                                                             const uint32_t *__restrict__ seg_list,
                                                             const unsigned long long *__restrict__ n_seg_ptr,
                                                             uint32_t *__restrict__ keys,
                                                             uint32_t *__restrict__ vals, PlaceParams pp,
                                                             uint32_t *__restrict__ long_list,
                                                             unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t s_ring[65 * 64];  // [slot][lane]: hit counts of the last TW + 1 processed probes
    const uint32_t lane = threadIdx.x;
    const uint64_t n_seg = *n_seg_ptr;
    const uint32_t RW = min(rp.tstar, 64u) + 1u;
    for (uint64_t base = (uint64_t)blockIdx.x * 64u; base < n_seg; base += (uint64_t)gridDim.x * 64u) {
        const uint64_t sidx = base + lane;
        const bool have = sidx < n_seg;
        uint32_t g0 = 0, g_end = 0;
        bool window_cut = false;  // the walk may end at the end of a sharded call's window instead of the chunk's
        if (have) {
            g0 = seg_list[sidx];
            const uint32_t chunk_end = rp.ch.pbase[chunk_of(rp.ch, g0) + 1];
            g_end = min(chunk_end, rp.win_end(g0));
            window_cut = g_end < chunk_end;
        }
        for (uint32_t r = 0; r < RW; ++r) s_ring[r * 64u + lane] = 0;
        uint32_t quiet = 0, mx = 0, bound = 0, n_probes = 0, wsum = 0, head = 0, steps = 0, g = g0, n_hit = 0;
        unsigned long long sum = 0;
        bool done = !have, by_quiet = false;
        while (!done && g < g_end && steps < kLaneWalk) {
            const uint32_t f = p_filt[g];
            ++g;
            ++steps;
            const bool hit = f >= 1u && f < kPending;
            if (!hit && f != 0u) continue;  // skipped probes (N, cardinality) are not processed
            if (!hit) {
                if (++quiet >= rp.tstar) {  // t* quiet probes: every arm has been retired, the segment is over
                    done = true;
                    by_quiet = true;
                    break;
                }
            } else {
                quiet = 0;
            }
            const uint32_t v = hit ? f : 0u;
            ++n_probes;
            n_hit += hit ? 1u : 0u;
            const uint32_t at = head * 64u + lane;
            wsum += v - s_ring[at];
            s_ring[at] = v;
            head = head + 1u == RW ? 0u : head + 1u;
            bound = max(bound, wsum);
            mx = max(mx, v);
            sum += v;
        }
        if (g >= g_end) done = true;
        if (have && done) {
            if (rp.tstar > 64u) bound = 0xFFFFFFFFu;  // no estimate for huge gap settings: largest tier
            bool tail_up;
            int tier = place_tier(bound, sum, n_probes, pp, &tail_up);
            if (mx > 1 && pp.force_tier > tier) tier = min(pp.force_tier, kTiers);
            if ((by_quiet || !window_cut) && segment_is_barren(pp, n_hit, g - g0)) tier = kTierBarren;
            if (tail_up && tier != kTierBarren) atomicAdd(&ctr[CT_TAIL_UP], 1ull);
            keys[sidx] = placement_key(tier, sum, g0);
            vals[sidx] = g0;
            if (pp.seg_info)
                pp.seg_info[sidx] = make_uint2(sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum,
                                               (g - g0) | ((by_quiet || !window_cut) ? 0x80000000u : 0u));
            if (pp.stats) {
                atomicAdd(&ctr[CT_TPROBES1 + tier - 1], (unsigned long long)n_hit);
                atomicAdd(&ctr[CT_THITS1 + tier - 1], sum);
            }
        }
        const unsigned long long lm = __ballot(have && !done);
        if (lm) {
            const int leader = __ffsll((long long)lm) - 1;
            unsigned long long at = 0;
            if ((int)lane == leader) at = atomicAdd(&ctr[CT_LONGSEG], (unsigned long long)__popcll(lm));
            at = __shfl(at, leader);
            if (have && !done) long_list[at + __popcll(lm & ((1ull << lane) - 1ull))] = (uint32_t)sidx;
        }
    }
}

// One wave per segment: the entries idx_list[0 .. *n_ptr) of the segment list (all of it when idx_list is null).
__global__ __launch_bounds__(64) void seg_stats_kernel(RunParams rp, const uint32_t *__restrict__ p_filt,
                                                       const uint32_t *__restrict__ seg_list,
                                                       const unsigned long long *__restrict__ n_ptr,
                                                       const uint32_t *__restrict__ idx_list,
                                                       uint32_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals, PlaceParams pp,
                                                       unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t s_ext[64 + 64];  // [0,TW): hit counts of the previous processed probes
    const int lane = threadIdx.x;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint64_t n_items = *n_ptr;
    const uint32_t TW = min(rp.tstar, 64u);
    for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint64_t sidx = idx_list ? (uint64_t)idx_list[item] : item;
        const uint32_t g0 = seg_list[sidx];
        const int c = chunk_of_uniform(rp.ch, g0);
        const uint32_t g_end = min(rp.ch.pbase[c + 1], rp.win_end(g0));
        const bool window_cut = g_end < rp.ch.pbase[c + 1];
        uint32_t quiet = 0, mx = 0, bound = 0, n_probes = 0, n_hit = 0, g_stop = g_end, g_after_hit = g0 + 1u;
        unsigned long long sum = 0;
        bool done = false;
        s_ext[lane] = 0;
        lds_barrier();
        // the next batch's hit counts are in flight while this one is processed: a long segment's walk is a chain
        // of dependent round trips (64 probes each) and sets the duration of the whole launch
        uint32_t f_next = g0 + (uint32_t)lane < g_end ? p_filt[g0 + lane] : kSkipN;
        for (uint32_t g = g0; g < g_end && !done; g += 64) {
            const uint32_t f = f_next;
            f_next = g + 64u + (uint32_t)lane < g_end ? p_filt[g + 64u + lane] : kSkipN;
            const unsigned long long hm = __ballot(f >= 1u && f < kPending);
            const unsigned long long qm = __ballot(f == 0u);
            if (!(hm | qm)) continue;  // 64 skipped probes (cardinality, N): nothing is processed, nothing changes
            unsigned long long live = ~0ull;  // probes of this batch that belong to the segment
            // The segment ends with the t*-th quiet probe in a row (skipped probes neither count nor interrupt,
            // a hit restarts the count).  Every lane prices the quiet run that ends at its own probe -- no walk
            // from hit to hit: in a dense array with interleaved quiet probes that scalar walk, 40-odd dependent
            // steps per batch, was the whole cost of placing the longest segment.
            {
                const unsigned long long hb = hm & lt_mask;  // hits before this lane
                const int lh = hb ? 63 - __clzll((long long)hb) : -1;
                const unsigned long long above_lh = lh < 0 ? ~0ull : (lh == 63 ? 0ull : ~((2ull << lh) - 1ull));
                const uint32_t run = (uint32_t)__popcll(qm & (lt_mask | (1ull << lane)) & above_lh) + (lh < 0 ? quiet : 0u);
                const unsigned long long term = __ballot(((qm >> lane) & 1ull) && run >= rp.tstar);
                if (term) {
                    // the run that reaches t* starts behind the hit at lh (of the terminating lane): only the
                    // probes up to that hit still belong to the segment
                    const uint32_t pos = (uint32_t)(__shfl(lh, __ffsll((long long)term) - 1) + 1);
                    done = true;
                    // (exactly behind the segment's last hit-probe: the barren tests want an upper bound of the span, the
                    // cutting into ranges must never place a cut on a hit-probe of the NEXT segment)
                    g_stop = pos ? g + pos : g_after_hit;
                    live = (1ull << pos) - 1ull;  // pos <= 63
                } else {
                    const int last = hm ? 63 - __clzll((long long)hm) : -1;
                    if (last >= 0) g_after_hit = g + (uint32_t)last + 1u;
                    const unsigned long long above = last < 0 ? ~0ull : (last == 63 ? 0ull : ~((2ull << last) - 1ull));
                    quiet = (uint32_t)__popcll(qm & above) + (last < 0 ? quiet : 0u);
                }
            }
            const unsigned long long procm = (hm | qm) & live;
            const bool proc = (procm >> lane) & 1ull;
            const uint32_t v = ((hm & live) >> lane) & 1ull ? f : 0u;
            const uint32_t r = (uint32_t)__popcll(procm & lt_mask);
            const uint32_t n_proc = (uint32_t)__popcll(procm);
            n_probes += n_proc;
            n_hit += (uint32_t)__popcll(hm & live);
            if (proc) s_ext[TW + r] = v;
            lds_barrier();
            uint32_t wsum = 0;
            if (proc)
                for (uint32_t d = 0; d <= TW; ++d) wsum += s_ext[TW + r - d];
            uint32_t m = v, wm = wsum;
            unsigned long long sv = v;
            for (int off = 32; off > 0; off >>= 1) {
                sv += __shfl_down(sv, off);
                m = max(m, (uint32_t)__shfl_down(m, off));
                wm = max(wm, (uint32_t)__shfl_down(wm, off));
            }
            sum += __shfl(sv, 0);
            mx = max(mx, (uint32_t)__shfl(m, 0));
            bound = max(bound, (uint32_t)__shfl(wm, 0));
            const uint32_t keep = (uint32_t)lane < TW ? s_ext[n_proc + lane] : 0u;
            lds_barrier();
            if ((uint32_t)lane < TW) s_ext[lane] = keep;
            lds_barrier();
        }
        if (rp.tstar > 64u) bound = 0xFFFFFFFFu;
        if (lane == 0) {
            bool tail_up;
            int tier = place_tier(bound, sum, n_probes, pp, &tail_up);
            if (mx > 1 && pp.force_tier > tier) tier = min(pp.force_tier, kTiers);
            if ((done || !window_cut) && segment_is_barren(pp, n_hit, min(g_stop, g_end) - g0)) tier = kTierBarren;
            if (tail_up && tier != kTierBarren) atomicAdd(&ctr[CT_TAIL_UP], 1ull);
            keys[sidx] = placement_key(tier, sum, g0);
            vals[sidx] = g0;
            if (pp.seg_info)
                pp.seg_info[sidx] = make_uint2(sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum,
                                               (min(g_stop, g_end) - g0) | ((done || !window_cut) ? 0x80000000u : 0u));
            if (pp.stats) {
                atomicAdd(&ctr[CT_TPROBES1 + tier - 1], (unsigned long long)n_hit);
                atomicAdd(&ctr[CT_THITS1 + tier - 1], sum);
            }
        }
        lds_barrier();
    }
}

// Barren by POSITION.  An arm's right segment is built from a chain of hits x_0 < x_1 < ... (one per hit-probe at most) with
// x_{j+1} < x_j + k + threshold (src/automaton.rs:68-70 with right.end = x_j + k), and it is reported only when
// x_m + k - x_0 >= M.  With buckets of w = k + thr_max positions (thr_max: the largest threshold any arm of the segment can
// have, as in segment_is_barren) every link of a chain stays in its bucket or moves to the next one, so an arm that reaches M
// leaves a RUN of at least floor((M - k) / w) + 1 consecutive occupied buckets among the segment's hits.  No such run =>
// the segment emits nothing.  That is the fate of the bursts of interspersed repeats, which are most of the extension's
// work at genome scale: a probe inside a repeat hits a hundred other copies, every copy collects a few hundred bases of
// hits over the few dozen probes of the burst, the copies are kilobases apart -- hundreds of arms per probe and not one
// duplication.  Tandem arrays and real duplications keep their runs and are run as before.
// One WAVE per segment: the hits' buckets set bits of a hashed LDS bitmap (BITS bits; a collision can only make a bucket look
// occupied that is not, i.e. a run look longer -- the test stays sound, it only proves a little less), then every hit
// asks whether the need - 1 buckets behind its own are all occupied.  Order-free, no barrier between waves, a few KB of
// LDS per wave (the continuation filter of round 2 answered a related question probe by probe, a wave per segment with
// barriers per probe, and cost more than it saved).  Segments of more than max_hits hits are left alone.
template <class PosT, int BITS>
__global__ __launch_bounds__(64) void cluster_barren_kernel(RunParams rp, PlaceParams pp,
                                                            const unsigned long long *__restrict__ row_off,
                                                            const PosT *__restrict__ hits,
                                                            const uint32_t *__restrict__ seg_list,
                                                            const unsigned long long *__restrict__ n_seg_ptr,
                                                            uint32_t *__restrict__ keys, uint32_t min_hits, uint32_t max_hits,
                                                            unsigned long long *__restrict__ cursor,
                                                            unsigned long long *__restrict__ ctr) {
    static_assert((BITS & (BITS - 1)) == 0 && BITS >= 2048, "bitmap size");
    constexpr uint32_t kWords = BITS / 32, kShift = 32 - __builtin_ctz((unsigned)BITS);
    __shared__ uint32_t s_bits[kWords];
    const uint32_t lane = threadIdx.x;
    const uint64_t n_seg = *n_seg_ptr;
    uint32_t n_barren = 0;
    auto bit_of = [&](uint32_t b) { return (b * 2654435761u) >> kShift; };
    for (;;) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, 64ull);
        base = lane_of(base, 0u);
        if (base >= n_seg) break;
        // the 64 segments of the batch side by side: key, hit total, where its rows are (most are not this launch's: already
        // barren, another size class, cut by a sharded window); the candidates are then walked one after the other, their
        // set-up already in registers
        const uint64_t sj = base + lane;
        bool cand = false;
        uint32_t key_l = 0, span_l = 0;
        unsigned long long lo_l = 0, hi_l = 0;
        if (sj < n_seg) {
            key_l = keys[sj];
            const uint2 info = pp.seg_info[sj];
            span_l = info.y & 0x7FFFFFFFu;
            cand = (key_l >> 29) < (uint32_t)kTiers && (info.y >> 31) && info.x >= min_hits && info.x <= max_hits;
            if (cand) {
                const uint32_t g0 = seg_list[sj];
                lo_l = row_off[g0];
                hi_l = row_off[g0 + span_l];
                cand = hi_l > lo_l && hi_l - lo_l <= (unsigned long long)max_hits;
            }
        }
        unsigned long long todo = __ballot(cand);
        while (todo) {
            const uint32_t l = (uint32_t)(__ffsll((long long)todo) - 1);
            todo &= todo - 1ull;
            const uint32_t key = lane_of(key_l, l), span = lane_of(span_l, l);
            const unsigned long long lo = lane_of(lo_l, l);
            const uint32_t n = (uint32_t)(lane_of(hi_l, l) - lo);
            const unsigned long long len_left_max = (unsigned long long)span * pp.step + pp.k;
            const unsigned long long thr_max = max((unsigned long long)pp.G, len_left_max / 10ull);
            const unsigned long long w = thr_max + pp.k;
            const unsigned long long need = (pp.M - pp.k) / w + 1ull;  // consecutive occupied buckets an emitting arm leaves
            if (need < 2ull || need > 64ull) continue;                 // (one bucket proves nothing; M > k: the host has checked)
            // exact floor(x / w) through a double quotient and one correction (x < 2^53; a 64-bit integer division per hit
            // would be a hundred instructions)
            const double inv_w = 1.0 / (double)w;
            auto bucket_of = [&](unsigned long long x) -> uint32_t {
                unsigned long long q = (unsigned long long)((double)x * inv_w);
                const long long r = (long long)(x - q * w);
                q += r >= (long long)w ? 1ull : 0ull;
                q -= r < 0 ? 1ull : 0ull;
                return (uint32_t)q;
            };
            for (uint32_t j = lane; j < kWords; j += 64u) s_bits[j] = 0u;
            __builtin_amdgcn_wave_barrier();
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // (eight independent loads per lane in flight, then the bits: a load-set loop would pay one round trip per pass)
            for (uint32_t j0 = 0; j0 < n; j0 += 512u) {
                PosT xv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    xv[u] = j < n ? hits[lo + j] : (PosT)0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    if (j < n) {
                        const uint32_t bi = bit_of(bucket_of((unsigned long long)xv[u]));
                        atomicOr(&s_bits[bi >> 5], 1u << (bi & 31u));
                    }
                }
            }
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            bool found = false;
            for (uint32_t j0 = 0; j0 < n && !found; j0 += 512u) {
                PosT xv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    xv[u] = j < n ? hits[lo + j] : (PosT)0;
                }
                bool mine = false;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t j = j0 + (uint32_t)u * 64u + lane;
                    if (j < n) {
                        const uint32_t b = bucket_of((unsigned long long)xv[u]);
                        bool all = true;
                        for (uint32_t d = 1; d < (uint32_t)need && all; ++d) {
                            const uint32_t bi = bit_of(b + d);
                            all = (s_bits[bi >> 5] >> (bi & 31u)) & 1u;
                        }
                        mine = mine || all;
                    }
                }
                found = __ballot(mine) != 0ull;
            }
            __builtin_amdgcn_wave_barrier();
            if (!found) {
                if (lane == 0) keys[base + l] = (key & 0x1FFFFFFFu) | ((uint32_t)(kTierBarren - 1) << 29);
                ++n_barren;
            }
        }
    }
    if (lane == 0 && n_barren) atomicAdd(&ctr[CT_CLUSTER_BARREN], (unsigned long long)n_barren);
}

// ---- long segments as ranges that run side by side (option split) ---------------------------------------------------------
// The probes of a segment are strictly serial, and the longest segment of a pass is the floor of its extension.  But the arm
// list a tandem array leaves behind at some probe c is, some way into the array, a function of the last few thousand probes
// only: a run that starts with NO arm `warm` probes in front of c holds, at c, exactly the arms (and the family state) of the
// run that started at the segment's first probe -- when it does.  Whether it does is CHECKED, never assumed: the range in
// front of the cut and a warm-up that stops at the cut both write out what they hold there (validate_cuts_kernel compares),
// where a cut fails the ranges in front of it stand, the records of those behind it are dropped and the rest of the segment
// runs as one more run from the last checked state (the whole segment again when its first cut fails).
//   plan_ranges_kernel     one thread per segment: the long ones of the long-shape tiers (3, 6) are taken off their tier's
//                          list and cut at the first hit-probe at or behind every range_len-th probe
//   validate_cuts_kernel   one workgroup per cut: same arms (by creation number, every field), same family state
//   fixup_records_kernel   one thread per record slot: family ordinals of a range + the flushes of the ranges before it;
//                          records of a segment that failed -> void
// Range size by budget (option split_len = 0): every run holds a compute unit, so the number of runs is what the cutting
// may cost.  A segment of `span` probe positions gets round(span / C) ranges of one length.  split_tally_kernel counts, for
// each candidate C, the runs that cutting every eligible segment would make; split_pick_kernel takes the SMALLEST C whose
// count fits the budget (a small job gets small ranges -- its few long segments are its whole extension --, a genome-sized
// one large ranges); warm-up C positions within [2 048, 6 144]; a segment is cut when it is at least 2 C and at least 3
// warm-ups long.  The choice depends on the segments only: the same in every call over the same input and settings.
constexpr int kSplitCand = 12;
__device__ inline uint32_t split_len_of(int c) {
    constexpr uint32_t t[kSplitCand] = {2048, 3072, 4096, 6144, 8192, 12288, 16384, 24576, 32768, 49152, 65536, 98304};
    return t[c];
}
// (half a range was not enough at the middle sizes: with ranges of 6 144 probes -- what a shard of a genome-sized call gets --
// and 3 072 of warm-up 20 of 44 cut segments had a cut that did not hold; with 6 144 every cut of the unsharded call holds)
__device__ inline uint32_t split_warm_of(uint32_t C) { return min(max(C, 2048u), 6144u); }
struct SplitChoice {
    uint32_t range_len, warm, min_span, pad;
    unsigned long long runs[kSplitCand];
};
__device__ inline bool split_eligible(const RunParams &rp, uint32_t key, uint2 info) {
    const uint32_t tier = (key >> 29) + 1u;
    // (tiers 1 and 2 are one-wave kernels: a wave on its own passes a sparse probe several times faster than the long shape's
    // sixteen waves and their barrier -- cutting a yeast-sized input's longest tier-2 segment in two doubled its step; cutting
    // the one-wave segments of 12 288 probe positions and more left a GRCh38-sized step and its shards where they were:
    // DESIGN_HISTORY.md; tier 7's arms do not fit the long shape)
    if (tier < 3u || tier > 6u) return false;
    const uint32_t span = info.y & 0x7FFFFFFFu;
    if (!(info.y >> 31) || span < 128u) return false;  // (cut short by a shard window: left alone)
    // (creation numbers of a run: needle offset relative to the segment's first probe << 10 | hit index)
    return (unsigned long long)span * (unsigned long long)rp.step < (1ull << 22) - 2ull;
}
__global__ __launch_bounds__(256) void split_tally_kernel(RunParams rp, const unsigned long long *__restrict__ n_seg_ptr,
                                                         const uint32_t *__restrict__ keys, const uint2 *__restrict__ seg_info,
                                                         SplitChoice *__restrict__ choice) {
    const unsigned long long sj = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (sj >= *n_seg_ptr) return;
    const uint2 info = seg_info[sj];
    const uint32_t span = info.y & 0x7FFFFFFFu;
    if (span < 3u * 2048u || !split_eligible(rp, keys[sj], info)) return;
    const unsigned long long cost = (unsigned long long)span;
    for (int c = 0; c < kSplitCand; ++c) {
        const unsigned long long C = split_len_of(c);
        if (cost < 2ull * C || span < 3u * split_warm_of((uint32_t)C)) break;
        atomicAdd(&choice->runs[c], max(2ull, (cost + C / 2ull) / C));
    }
}
__global__ void split_pick_kernel(SplitChoice *choice, uint32_t budget) {
    int pick = kSplitCand - 1;
    for (int c = 0; c < kSplitCand; ++c)
        if (choice->runs[c] <= (unsigned long long)budget) {
            pick = c;
            break;
        }
    choice->range_len = split_len_of(pick);
    choice->warm = split_warm_of(split_len_of(pick));  // (E. coli-sized inputs: cuts with 1 024 probes of warm-up did not hold)
    choice->min_span = 3u * choice->warm;               // (two ranges of a shorter segment are each nearly the segment)
}

constexpr uint32_t kSplitBlockedMax = 2048;  // verdicts of earlier calls handed to one call
// what an earlier call of the index found out about a segment a cut of which did not hold
struct BlockedSeg {
    uint32_t g0;         // the segment (first probe, in this call's numbering)
    uint32_t range_len;  // at which range length (the verdict means nothing at another)
    uint32_t allowed;    // how many of its cuts, counted from the segment's start, are planned again (kAllCuts: all of them)
    uint32_t warm;       // the warm-up its ranges get from now on (0: the call's)
};
constexpr uint32_t kAllCuts = 0xFFFFFFFFu;
struct SplitParams {
    uint32_t range_len, warm, min_span;   // size of a range (probe positions; range_len = 0: cost units, as split_pick_kernel chose),
                                          // warm-up probes in front of a cut, shortest segment that is cut
    uint32_t max_runs, max_cuts, max_splits;
    uint32_t n_blocked;
    const BlockedSeg *blocked;            // segments a cut of which did not hold in an earlier call of the index
};
__global__ __launch_bounds__(256) void plan_ranges_kernel(RunParams rp, SplitParams sp, const uint32_t *__restrict__ p_filt,
                                                         const uint32_t *__restrict__ seg_list,
                                                         const unsigned long long *__restrict__ n_seg_ptr,
                                                         uint32_t *__restrict__ keys, const uint2 *__restrict__ seg_info,
                                                         unsigned long long *__restrict__ hdr,  // 0 runs, 1 cuts, 2 split segments
                                                         RangeRun *__restrict__ runs, uint2 *__restrict__ cuts,
                                                         SplitSeg *__restrict__ splits, const SplitChoice *__restrict__ choice) {
    const unsigned long long sj = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (sj >= *n_seg_ptr) return;
    if (!sp.range_len) {  // (hdr[3] is the runs' work cursor: hdr[4] tells the host which length was used)
        sp.range_len = choice->range_len;
        sp.warm = choice->warm;
        sp.min_span = max(sp.min_span, choice->min_span);
        if (sj == 0) hdr[4] = sp.range_len;
    } else if (sj == 0) {
        hdr[4] = sp.range_len;
    }
    const uint32_t key = keys[sj];
    const uint2 info = seg_info[sj];
    const uint32_t span = info.y & 0x7FFFFFFFu;
    if (span < sp.min_span || !split_eligible(rp, key, info)) return;
    const uint32_t g0 = seg_list[sj];
    // a segment a cut of which did not hold in an earlier call: its ranges start as far in front of their cuts as the oldest
    // arm at the failed cut asked for -- or, where that is further than a range is worth, only the cuts that held are planned again
    uint32_t warm = sp.warm;
    uint32_t n_cut_max = 0xFFFFFFFFu;
    for (uint32_t b = 0; b < sp.n_blocked; ++b) {
        const BlockedSeg v = sp.blocked[b];
        if (v.g0 == g0 && v.range_len == sp.range_len) {
            n_cut_max = min(n_cut_max, v.allowed);
            warm = max(warm, v.warm);
        }
    }
    // ranges of about range_len probe positions each, at least two, their cuts at equal shares of the segment; a segment whose
    // cuts held only up to some point in an earlier call keeps those cuts (same places) and runs the rest as its last range
    // (cuts at equal shares of positions + hits / w instead were measured at GRCh38 size and did not move the step: DESIGN_HISTORY.md)
    const unsigned long long total = span, unit = sp.range_len;
    if (total < 2ull * unit) return;
    const uint32_t n_r_all = (uint32_t)min(1024ull, max(2ull, (total + unit / 2ull) / unit));
    const uint32_t n_r = min(n_r_all, n_cut_max == kAllCuts ? n_r_all : n_cut_max + 1u);
    if (n_r < 2u) return;
    auto cut_of = [&](uint32_t j) -> uint32_t {  // first hit-probe at or behind the j-th share of the cost (0: none)
        uint32_t c = g0 + (uint32_t)(total / n_r_all * j);
        while (c < g0 + span) {
            const uint32_t f = p_filt[c];
            if (f >= 1u && f < kPending) return c;
            ++c;
        }
        return 0u;
    };
    {   // (every cut behind its predecessor, the first behind the segment's start)
        uint32_t before = g0;
        for (uint32_t j = 1; j < n_r; ++j) {
            const uint32_t c = cut_of(j);
            if (c <= before) return;
            before = c;
        }
    }
    const uint32_t n_runs = n_r;
    const uint32_t run_base = (uint32_t)atomicAdd(&hdr[0], (unsigned long long)n_runs);
    if (run_base + n_runs > sp.max_runs) {
        atomicAdd(&hdr[0], 0ull - (unsigned long long)n_runs);
        return;
    }
    const uint32_t cut_base = (uint32_t)atomicAdd(&hdr[1], (unsigned long long)(n_r - 1u));
    const uint32_t split = (uint32_t)atomicAdd(&hdr[2], 1ull);
    if (cut_base + n_r - 1u > sp.max_cuts || split >= sp.max_splits) {  // (sized together with max_runs: does not happen)
        atomicAdd(&hdr[0], 0ull - (unsigned long long)n_runs);
        atomicAdd(&hdr[1], 0ull - (unsigned long long)(n_r - 1u));
        atomicAdd(&hdr[2], 0ull - 1ull);
        return;
    }
    keys[sj] = (key & 0x1FFFFFFFu) | ((uint32_t)(kTierBarren - 1) << 29);  // off its tier's list
    splits[split] = SplitSeg{g0, run_base, n_r, cut_base, span, info.x, (key >> 29) + 1u, warm};
    uint32_t c_prev = g0;
    for (uint32_t j = 0; j < n_r; ++j) {
        const uint32_t c_next = j + 1u < n_r ? cut_of(j + 1u) : 0xFFFFFFFFu;
        RangeRun r{};
        r.g_begin = (j == 0u || c_prev - g0 <= warm) ? g0 : c_prev - warm;
        r.g_stop = c_next;
        r.g_seg0 = g0;
        r.emit_from = c_prev;
        r.flags = j + 1u == n_r ? kRunLast : 0u;
        r.split = split;
        runs[run_base + j] = r;
        // (what range j - 1 holds when it stops at this range's cut against what this range holds when it reaches it)
        if (j) cuts[cut_base + j - 1u] = make_uint2(run_base + j - 1u, run_base + j);
        c_prev = c_next;
    }
}

// (option debug = 2: per tier the placed segment with the most probe positions and the one with the most hits that was NOT cut
// -- top[2 t] and top[2 t + 1] = figure << 32 | segment)
__global__ __launch_bounds__(256) void top_uncut_kernel(const unsigned long long *__restrict__ n_seg_ptr, const uint32_t *__restrict__ keys,
                                                       const uint2 *__restrict__ seg_info, unsigned long long *__restrict__ top) {
    const unsigned long long sj = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (sj >= *n_seg_ptr) return;
    const uint32_t tier = keys[sj] >> 29;
    if (tier >= (uint32_t)kTiers) return;
    const uint2 info = seg_info[sj];
    atomicMax(&top[2u * tier], (unsigned long long)(info.y & 0x7FFFFFFFu) << 32 | sj);
    atomicMax(&top[2u * tier + 1u], (unsigned long long)info.x << 32 | sj);
}

template <uint32_t W>  // (words per dumped arm: kDumpWords)
__global__ __launch_bounds__(256) void validate_cuts_kernel(const uint2 *__restrict__ cuts, const uint32_t *__restrict__ run_meta,
                                                           const uint32_t *__restrict__ run_dump, uint32_t *__restrict__ cut_ok) {
    constexpr uint32_t Q = W / 4u;  // 16-byte quarters of an arm
    constexpr uint32_t kSlots = 16384;  // > 3 x kRunDumpCap
    __shared__ uint32_t s_tab[kSlots];
    __shared__ uint32_t s_ok, s_oldest;
    const uint2 cut = cuts[blockIdx.x];
    // (x: the run in front of the cut, its end state; y: the run behind it, its state at the cut)
    const uint32_t *ma = run_meta + (size_t)cut.x * 16, *mb = run_meta + (size_t)cut.y * 16 + 8;
    const uint32_t n = ma[0];
    const bool meta_ok = n == mb[0] && n <= kRunDumpCap && ma[2] == mb[2] && ma[3] == mb[3] && !ma[4] && !run_meta[(size_t)cut.y * 16 + 4];
    for (uint32_t j = threadIdx.x; j < kSlots; j += blockDim.x) s_tab[j] = 0u;
    if (threadIdx.x == 0) {
        s_ok = meta_ok ? 1u : 0u;
        s_oldest = 0xFFFFFFFFu;
    }
    __syncthreads();
    {   // the oldest arm the range in front of the cut holds there (its creation number: where in the segment it was born): a
        // run that is to hold it at the cut must start in front of that probe -- what the host sizes the next warm-up by
        const uint4 *da = reinterpret_cast<const uint4 *>(run_dump + (size_t)cut.x * 2 * kRunDumpCap * W);
        uint32_t oldest = 0xFFFFFFFFu;
        for (uint32_t j = threadIdx.x; j < min(n, kRunDumpCap); j += blockDim.x) oldest = min(oldest, da[Q * j].x);
        if (oldest != 0xFFFFFFFFu) atomicMin(&s_oldest, oldest);
    }
    if (meta_ok) {
        const uint4 *da = reinterpret_cast<const uint4 *>(run_dump + (size_t)cut.x * 2 * kRunDumpCap * W);
        const uint4 *db = reinterpret_cast<const uint4 *>(run_dump + ((size_t)cut.y * 2 + 1) * kRunDumpCap * W);
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
            uint32_t h = (da[Q * j].x * 2654435761u) >> 18;
            while (atomicCAS(&s_tab[h], 0u, j + 1u) != 0u) h = (h + 1u) & (kSlots - 1u);
        }
        __syncthreads();
        bool ok = true;
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
            const uint4 b0 = db[Q * j];
            uint32_t h = (b0.x * 2654435761u) >> 18;
            bool found = false;
            for (uint32_t probe = 0; probe < kSlots; ++probe) {
                const uint32_t e = s_tab[h];
                if (!e) break;
                const uint4 a0 = da[Q * (e - 1u)];
                if (a0.x == b0.x) {  // (creation numbers are unique within a dump)
                    found = a0.y == b0.y && a0.z == b0.z && a0.w == b0.w;
                    for (uint32_t q = 1; q < Q; ++q) {
                        const uint4 a = da[Q * (e - 1u) + q], b = db[Q * j + q];
                        found = found && a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
                    }
                    break;
                }
                h = (h + 1u) & (kSlots - 1u);
            }
            ok = ok && found;
        }
        if (!ok) s_ok = 0u;
    }
    __syncthreads();
    // (bit 0: the cut holds; above it: needle offset, counted from the segment's first probe, at which the oldest arm was born --
    // all ones: no arm)
    if (threadIdx.x == 0) cut_ok[blockIdx.x] = s_ok | ((s_oldest >> 10) << 1);
}

// run_fix[run]: what is added to the family ordinals of the run's records; ~0u: the run's records are dropped; ~0u - 1: not
// decided yet (left as they are for a later pass)
__global__ __launch_bounds__(256) void fixup_records_kernel(SdRec *__restrict__ recs, unsigned long long n, const uint32_t *__restrict__ run_fix) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SdRec &r = recs[i];
    if (r.g_start == kVoidStart || r.pad == 0u) return;
    const uint32_t f = run_fix[r.pad - 1u];
    if (f == 0xFFFFFFFEu) return;
    if (f == 0xFFFFFFFFu) r.g_start = kVoidStart;
    else r.fam_seq += f;
    r.pad = 0u;
}

// tier list lengths from the sorted placement keys (tier-1 = key >> 29): n_t = first index whose
// tier exceeds t, by bisection -- instead of one contended global atomic per segment
__global__ void tier_bounds_kernel(const uint32_t *__restrict__ sorted_keys,
                                   const unsigned long long *__restrict__ n_seg_ptr,
                                   unsigned long long *__restrict__ ctr) {
    const int t = threadIdx.x;  // 0..4
    if (t >= kTiers) return;
    const uint64_t n = *n_seg_ptr;
    auto first_ge = [&](uint32_t tier_idx) {  // first position with (key >> 29) >= tier_idx
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((sorted_keys[mid] >> 29) < tier_idx) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    ctr[CT_N1 + t] = first_ge((uint32_t)t + 1u) - first_ge((uint32_t)t);
}

// yardstick: sum over searched probes of ceil(log2(b_p + 1)), b_p = size of the
// reference's 8-mer bucket.  Untimed.
template <class SlotT>
__global__ __launch_bounds__(256) void yardstick_kernel(IndexView<SlotT> ix, RunParams rp,
                                                        const uint32_t *__restrict__ p_filt,
                                                        unsigned long long *__restrict__ ctr) {
    uint32_t g_end;
    const uint32_t g = rp.tile_of(blockIdx.x, 256u, g_end) + threadIdx.x;
    unsigned long long steps = 0;
    if (g < g_end && p_filt[g] != kSkipN) {
        const int c = chunk_of(rp.ch, g);
        const uint64_t s = rp.ch.start[c], L = rp.ch.len[c];
        const uint64_t i = (uint64_t)(g - rp.ch.pbase[c] + 1) * (uint64_t)rp.step;
        uint32_t first;
        const uint32_t md = rp.mode_of(c);
        const uint64_t q = probe_key(ix.text, s, L, i, rp.k, (md & 2u) != 0u, (md & 1u) != 0u, &first);
        uint32_t c8;
        if (cache8_index((uint32_t)(q >> (3 * (ix.kk - kCacheLen))), c8)) {
            const uint64_t b = (uint64_t)ix.c8hi[c8] - (uint64_t)ix.c8lo[c8];
            uint64_t v = 1;
            while (v < b + 1) {
                v <<= 1;
                ++steps;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) steps += __shfl_down(steps, off);
    if ((threadIdx.x & 63) == 0 && steps) atomicAdd(&ctr[CT_BISECT], steps);
}

}  // namespace asgart
