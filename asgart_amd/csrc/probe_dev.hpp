// probe_dev.hpp -- the probe search: per probe its suffix-array interval and the number of occurrences the hit filter
// (HitRule, device_base.hpp) keeps.
//
//   probe_count_kernel      a wave per tile of 256 probes: text window and position bits staged in LDS, the probes the
//                           bits do not answer compacted and looked up; small intervals counted, large ones marked
//   collect_pending_kernel  the marks -> big_list and rank_list
//   rank_count_kernel       a thread per entry of rank_list: the kept count by bisection of the position-sorted list;
//                           rows to fill go on to big_list or to the ranked list
//   big_count_kernel        a wave per 64 entries of big_list: the interval streamed, early exit at max_cardinality + 1
//   raw_hits_kernel         asgart_stats.raw_hits, when the statistics are asked for
//   yardstick_kernel        the bench's bisection yardstick (untimed)
// COUNT = true instantiations are the accounting pass behind bench.py's `kernel_algorithmic_bytes`.
//
// Reference semantics: src/automaton.rs:57-216 (see DESIGN.md for the proof that a run of ceil(G/step) processed zero-hit
// probes empties the arm list, which is what makes segments independent).
#pragma once

#include "device_base.hpp"

namespace asgart {

// ---------------------------------------------------------------- K1 ---------
// Probe search: one wave per tile of 256 consecutive probes, four probes per lane.
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
    auto lookup = [&](uint32_t g_, uint64_t q_, uint64_t q2_, const ProbeAt &at_, const uint64_t *lrn_) {
        const bool reverse = (at_.md & 2u) != 0u, complement = (at_.md & 1u) != 0u;
        const HitRule hr = hit_rule(at_);
        uint64_t lo, hi;
        ProbeRef pr;  // (read only by probes of more than 42 bases)
        pr.p = reverse ? ix.text + at_.s + at_.L - 1u - at_.i : ix.text + at_.s + at_.i;
        pr.dir = reverse ? -1 : 1;
        pr.comp = complement;
        const bool all_occurrences = kmer_range(ix, q_, q2_, pr, lo, hi, cb);
        const uint64_t raw = hi - lo;
        cb.looked_up(raw);
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
            const bool only_self = all_occurrences && raw == 1 && at_.md == 0u;
            bool any = false;  // an occurrence that could be kept, whatever chunk the probe came in (a reversed needle's
                               // `m.start != i` compares a text position with a chunk offset: left out)
            for (uint64_t r = lo; r < hi && !only_self; ++r) {
                cb.rd_sa(sizeof(SlotT));
                const uint64_t x = ix.sa[r];
                cnt += hr.keeps(x) ? 1u : 0u;
                if (reverse) any |= x >= hr.thr;
            }
            if (!reverse) any = cnt != 0u;
            if (!COUNT) p_filt[g_] = cnt > rp.C ? kSkipCard : cnt;
            cb.wr(4);
            if constexpr (!COUNT) {
                // learned position bits: no occurrence of this probe's k-mer can ever be kept at this text position
                if (lrn_ && all_occurrences && !any) {
                    const uint64_t p = (uint64_t)probe_bit_pos(at_, k);
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
        const ProbeAt at0 = probe_at(rp, c0, gb);  // probe gb; probe gb + t lies t * H further into the same chunk
        auto at_of = [&](uint32_t t) { return ProbeAt{at0.i + (uint64_t)t * (uint64_t)H, at0.s, at0.L, at0.md}; };
        const uint32_t md = at0.md;  // (the orientation of the chunk's pass)
        const bool reverse = (md & 2u) != 0u, complement = (md & 1u) != 0u;
        const uint64_t *const pbits = rp.pbits[rp.pass_of(c0)];
        const uint64_t s = at0.s, L = at0.L, i0 = at0.i;
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
            // text positions the probes cover: direct  s + i0 + t H ;  reversed  s + L - i0 - k - t H  (the lowest is the
            // tile's first probe's, or its last's)
            const long long p_first = probe_bit_pos(at_of(reverse ? (uint32_t)kProbeBlock - 1u : 0u), k);
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
                if (first != 4u && pbits) {  // the bit of the text position the probe covers
                    const uint32_t b = (uint32_t)(probe_bit_pos(at_of(t), k) - pb_lo);
                    pass = (s_pb[b >> 5] >> (b & 31u)) & 1u;
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
            lookup(gb + t, key_of(t), 0ull, at_of(t), pbits);
        }
    } else {
        // the tile straddles a chunk boundary (or the probes are longer than one key word): every probe on its own
#pragma unroll 1
        for (int u = 0; u < kProbeSub; ++u) {
            const uint32_t g = gb + lane + (uint32_t)u * kProbeThreads;
            if (g >= g_end) continue;
            const int c = chunk_of(rp.ch, g);
            const ProbeAt at = probe_at(rp, c, g);
            const uint64_t *const pbits = rp.pbits[rp.pass_of(c)];
            uint32_t first = 0;
            uint64_t q2 = 0;
            const uint64_t q = probe_key(ix.text, at.s, at.L, at.i, k, (at.md & 2u) != 0u, (at.md & 1u) != 0u, &first, &q2);
            cb.rd((uint32_t)k);
            bool pass = true;
            if (first != 4u && pbits) {
                const uint64_t p = (uint64_t)probe_bit_pos(at, k);
                cb.rd(8);
                pass = (pbits[p >> 6] >> (p & 63u)) & 1ull;
            }
            if (screen(g, first, pass, at.md)) lookup(g, q, q2, at, pbits);
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
        for (int j = 0; j < (int)LA_COUNT; ++j) {  // the looked-up probes' loads by array (asgart_lookup_account)
            unsigned long long a = cb.la[j];
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
            if (lane == 0 && a) atomicAdd(&ctr[CT_LOOKUP_ACCT + j], a);
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
            const HitRule hr = hit_rule(probe_at(rp, g));
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
            // kept: x >= thr, less self where it lies there and is in the list (a reversed pass; a direct one has self < thr)
            uint64_t cnt = R - first_ge(hr.thr);
            if (hr.self >= hr.thr) {
                const uint64_t j = first_ge(hr.self);
                if (j < R && (uint64_t)a[j] == hr.self) --cnt;
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
        uint32_t g = 0;
        unsigned long long lo = 0, hi = 0;
        HitRule hr = {0ull, 0ull};
        if (lane < np) {
            g = big_list[e0 + lane];
            hr = hit_rule(probe_at(rp, g));
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
            const unsigned long long lo_p = lane_of(lo, p), hi_p = lane_of(hi, p);
            const HitRule hr_p = lane_of(hr, p);
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
                    const bool keep = r < hi_p && hr_p.keeps(x[u]);
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
                const ProbeAt at = probe_at(rp, g);
                const bool reverse = (at.md & 2u) != 0u, complement = (at.md & 1u) != 0u;
                uint32_t first = 0;
                uint64_t q2 = 0, lo, hi;
                const uint64_t q = probe_key(ix.text, at.s, at.L, at.i, rp.k, reverse, complement, &first, &q2);
                ProbeRef pr;
                pr.p = reverse ? ix.text + at.s + at.L - 1u - at.i : ix.text + at.s + at.i;
                pr.dir = reverse ? -1 : 1;
                pr.comp = complement;
                kmer_range(ix, q, q2, pr, lo, hi);
                raw = (uint32_t)(hi - lo);
            }
            sum += raw;
        }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(out, sum);
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
        const ProbeAt at = probe_at(rp, g);
        uint32_t first;
        const uint64_t q = probe_key(ix.text, at.s, at.L, at.i, rp.k, (at.md & 2u) != 0u, (at.md & 1u) != 0u, &first);
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
