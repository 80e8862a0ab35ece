// extend_heavy_dev.hpp -- "K4b", the extension kernel of the heavy tiers (2 / 4 / 6 beyond the staging area, 7).
// Block-cooperative: ONE workgroup (NT = 256 or 1024 threads) per segment, for
// the segments whose live-arm bound does not fit the one-wave kernel.  At genome scale these are
// dense-repeat clusters and satellite tails: hundreds of hits per probe, hundreds to thousands of
// live arms, most of them single-hit arms that die t* probes after they were born.
//
// Same results as extend_kernel, different bookkeeping:
//   * arms live in SLOTS; a dead arm's slot goes on a free list and is reused, so there is no
//     order-preserving compaction.  "First matching arm in list order" (src/automaton.rs:67-78)
//     is the accepting arm with the smallest CREATION NUMBER (list order == creation order), so
//     slot order is irrelevant.
//   * per probe: (0) clear hash heads, (1) hash narrow arms by bucket(re) / list wide arms,
//     (2) one thread per hit: two buckets + wide list -> best (creation number, slot),
//     (3) ExtendArm = atomicMax of the hit index on the slot, NewArm = slot from the free list in
//     hit order, (4) apply / age / retire in place.
//   * MODE 2 keeps the arm arrays in an HBM scratch slice per workgroup (up to 16384
//     live arms); the per-probe candidate index stays in LDS.
#pragma once

#include "extend_common_dev.hpp"

namespace asgart {

constexpr int kHeavyThreads = 512;   // heavy tiers (1024 threads would cap VGPRs at 128 -> spills)
constexpr int kMidThreads = 256;     // mid tier: 4 waves per segment, several workgroups per CU

// MODE 0: every arm field in LDS.  MODE 1 ("hybrid"): everything a probe reads or updates (ls, le,
// re, thr, seq, gap, pend) in LDS; rs, written once at creation and read once at retirement, in an
// HBM scratch slice (no global access on the per-probe path: a pending global store would stall
// every workgroup barrier); 16-bit gap/pend and an index-form wide list -> ~1.9x the capacity.
// MODE 2: all fields in HBM scratch (last resort, up to 16384 live arms).
// atomic max on a 32-bit or (LDS, packed pairs) 16-bit element
__device__ inline void pend_max(uint32_t *a, uint32_t idx, uint32_t v) { atomicMax(&a[idx], v); }
__device__ inline void pend_max(uint16_t *a, uint32_t idx, uint32_t v) {
    // two 16-bit elements per word: the other half must be left untouched -> CAS loop
    uint32_t *w = reinterpret_cast<uint32_t *>(a) + (idx >> 1);
    const uint32_t sh = (idx & 1u) * 16u;
    uint32_t old = *w;
    for (;;) {
        const uint32_t cur = (old >> sh) & 0xFFFFu;
        if (cur >= v) break;
        const uint32_t upd = (old & ~(0xFFFFu << sh)) | (v << sh);
        const uint32_t prev = atomicCAS(w, old, upd);
        if (prev == old) break;
        old = prev;
    }
}

template <class PosT, int CAP, int NT, int MODE>
__global__ __launch_bounds__(NT) void extend_heavy_kernel(ExtParams<PosT> P) {
    constexpr int NW = NT / 64;
    constexpr bool PACKED_WIDE = MODE == 0;
    constexpr int HCAP = MODE != 2 ? CAP : 1;  // hot fields in LDS
    constexpr int CCAP = MODE == 0 ? CAP : 1;  // cold field (rs) in LDS
    // MODE 2: the capacity is a launch parameter (P.heavy_cap: max_cardinality * (ceil(G / step) + 1) bounds the
    // live arms of ANY segment -- every live arm was created or extended within the last t* + 1 processed probes,
    // at most max_cardinality of them per probe), slots are 32-bit and the per-arm index lists live in the HBM slice
    // as well; CAP is ignored.
    const uint32_t cap_rt = MODE == 2 ? P.heavy_cap : (uint32_t)CAP;
    constexpr uint32_t kSlotBits = MODE == 2 ? 24u : 20u;  // (creation number << kSlotBits) | slot
    constexpr uint32_t kSlotMask = (1u << kSlotBits) - 1u;
    using IdxT = typename std::conditional<MODE == 2, uint32_t, uint16_t>::type;
    constexpr uint32_t kEndIdx = MODE == 2 ? 0xFFFFFFFFu : 0xFFFFu;
    __shared__ PosT l_ls[HCAP], l_re[HCAP], l_le[HCAP], l_rs[CCAP];
    // gap and pend are 16-bit in the hybrid tier (gap saturates; the host only uses that tier when
    // G and max_cardinality fit): 24 B of LDS per arm instead of 32
    using SmallT = typename std::conditional<MODE == 1, uint16_t, uint32_t>::type;
    constexpr uint32_t kGapMax = MODE == 1 ? 0xFFFFu : 0xFFFFFFFFu;
    __shared__ uint32_t l_thr[HCAP], l_seq[HCAP];
    __shared__ SmallT l_gap[HCAP], l_pend[HCAP];
    PosT *s_ls = l_ls, *s_le = l_le, *s_rs = l_rs, *s_re = l_re;
    uint32_t *s_thr = l_thr, *s_seq = l_seq;
    SmallT *s_gap = l_gap, *s_pend = l_pend;
    IdxT *g_next = nullptr, *g_free = nullptr, *g_widx = nullptr;
    if constexpr (MODE != 0) {
        const size_t bytes = (size_t)cap_rt * (4 * sizeof(PosT) + (MODE == 2 ? 7 : 4) * sizeof(uint32_t));
        char *b = P.scratch + (size_t)blockIdx.x * bytes;
        PosT *g0p = reinterpret_cast<PosT *>(b);
        s_rs = g0p + 2 * (size_t)cap_rt;
        if constexpr (MODE == 2) {
            s_ls = g0p;
            s_le = g0p + cap_rt;
            s_re = g0p + 3 * (size_t)cap_rt;
            s_gap = reinterpret_cast<SmallT *>(g0p + 4 * (size_t)cap_rt);
            s_thr = reinterpret_cast<uint32_t *>(s_gap + cap_rt);
            s_seq = s_thr + cap_rt;
            s_pend = reinterpret_cast<SmallT *>(s_seq + cap_rt);
            g_next = reinterpret_cast<IdxT *>(s_pend + cap_rt);
            g_free = g_next + cap_rt;
            g_widx = g_free + cap_rt;
        }
    }
    constexpr uint32_t HT = MODE == 2 ? 8192u : (CAP <= 1024 ? 1024u : (MODE == 1 ? 2048u : (CAP <= 4608 ? 4096u : 8192u)));
    constexpr uint32_t WCAP = PACKED_WIDE ? (uint32_t)CAP : 1u;
    __shared__ uint32_t s_head[HT];
    __shared__ uint16_t l_next[MODE == 2 ? 1 : CAP];
    __shared__ uint16_t l_free[MODE == 2 ? 1 : CAP];  // stack of empty slots below the high-water mark
    __shared__ PosT s_ivlo[WCAP];     // wide arm w accepts x iff (x - s_ivlo[w]) < s_ivw[w]
    __shared__ uint32_t s_ivw[WCAP];
    __shared__ unsigned long long s_wkey[WCAP];  // (creation number << 20) | slot of wide arm w
    __shared__ uint16_t l_widx[(PACKED_WIDE || MODE == 2) ? 1 : CAP];  // index form of the wide list
    IdxT *s_next, *s_free, *s_widx;
    if constexpr (MODE == 2) {
        s_next = g_next; s_free = g_free; s_widx = g_widx;
    } else {
        s_next = l_next; s_free = l_free; s_widx = l_widx;
    }
    __shared__ PosT s_hits[kHitBatch];
    __shared__ unsigned long long s_best[NT];  // per hit: (creation number << 20) | slot, or ~0
    __shared__ uint32_t s_nwide, s_nfreed;
    __shared__ uint32_t s_wcnt[NT / 64];
    __shared__ unsigned long long s_bcast;
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const RunParams &rp = P.rp;
    const uint64_t n_seg = *P.n_seg_ptr;
    const uint32_t k = (uint32_t)rp.k, step = (uint32_t)rp.step, G = rp.G;
    const uint32_t thr0 = arm_threshold(k, G);
    const uint32_t bsh = bucket_shift(G, k);  // a hit meets <= 2 buckets
    const uint32_t cap_eff = min(cap_rt, P.cap_limit);
    RecAlloc rec_alloc;
    wg_begin(P);
    PROF_DECL;

    for (;;) {
        if (tid == 0) s_bcast = atomicAdd(P.cursor, 1ull);
        __syncthreads();
        const unsigned long long seg = s_bcast;
        __syncthreads();
        if (seg >= n_seg) break;
        const uint32_t g0 = P.seg_list[seg];
        if (tid == 0) {
            heartbeat(P, g0, 0u);
            seg_clock(P);
        }
        PROF_SEG_BEGIN();
        const SegHeader sg = load_segment(rp, g0);
        // block-uniform state: A live arms in slots [0,H), n_free of them empty (on s_free)
        uint32_t A = 0, H = 0, n_free = 0, quiet = 0, fam_seq = 0, next_seq = 0;
        if (tid == 0) s_nfreed = 0;
        bool overflow = false, done = false, fam_open = false;

        auto emit_records = [&](bool emit, PosT ls, PosT le, PosT rs, PosT re, uint32_t seq) {
            const unsigned long long em = __ballot(emit);
            if (!em) return;
            const unsigned long long at = rec_slot(rec_alloc, P, em, lane);
            if (emit) write_record(P, at, g0, fam_seq, seq, 0u, sg.cs, sg.cl, sg.rev, ls, le, rs, re);
        };
        // Age every live arm by `add` (unless `extended` applies first), retire in place the ones
        // whose gap reaches G.  i, off, row, from_lds describe the probe that may have extended
        // arms (with_pend); block-uniform on exit: A, n_free, fam_seq, next_seq, H.
        auto age_and_retire = [&](uint32_t add, bool with_pend, uint64_t i, uint32_t off,
                                  unsigned long long row, bool from_lds) {
            // s_nfreed was cleared at least one barrier ago (probe start / previous call's end)
            for (uint32_t j0 = 0; j0 < H; j0 += NT) {
                const uint32_t j = j0 + tid;
                bool dead = false;
                PosT ls = 0, le = 0, rs = 0, re = 0;
                uint32_t sq = kNoSeq;
                if (j < H && (sq = s_seq[j]) != kNoSeq) {
                    const uint32_t pd = with_pend ? s_pend[j] : 0u;
                    if (pd) {
                        s_pend[j] = 0;
                        const PosT x = from_lds ? s_hits[off + pd - 1u] : P.hits[row + pd - 1u];
                        s_re[j] = (PosT)(x + k);
                        s_le[j] = (PosT)(i + k);
                        s_thr[j] = arm_threshold((uint64_t)(i + k) - (uint64_t)s_ls[j], G);
                        s_gap[j] = 0;
                    } else {
                        const uint32_t gp = s_gap[j];
                        const uint64_t sum_g = (uint64_t)gp + add;
                        const uint32_t ng = sum_g > kGapMax ? kGapMax : (uint32_t)sum_g;
                        s_gap[j] = (SmallT)ng;
                        if (ng >= G) {
                            dead = true;
                            ls = s_ls[j]; le = s_le[j]; rs = s_rs[j]; re = s_re[j];
                            s_seq[j] = kNoSeq;
                            s_free[n_free + atomicAdd(&s_nfreed, 1u)] = (IdxT)j;
                        }
                    }
                }
                emit_records(dead && (uint64_t)(re - rs) >= rp.M, ls, le, rs, re, sq);
            }
            __syncthreads();
            const uint32_t nd = s_nfreed;
            __syncthreads();
            if (tid == 0) s_nfreed = 0;  // visible after the next barrier, before the next use
            A -= nd;
            n_free += nd;
            if (A == 0) {  // every slot is empty again
                H = 0;
                n_free = 0;
            } else if (H > 2u * A + 128u) {
                // Mostly holes (a long segment past its peak): pack the live arms into [0, A) so
                // that the per-probe loops run over A slots again.  Slot order is free (matching
                // goes by creation number).  Iteration by iteration: read, barrier, write below.
                uint32_t w = 0;
                for (uint32_t j0 = 0; j0 < H; j0 += NT) {
                    const uint32_t j = j0 + tid;
                    const bool live = j < H && s_seq[j] != kNoSeq;
                    PosT ls = 0, le = 0, rs = 0, re = 0;
                    uint32_t gp = 0, th = 0, sq = kNoSeq;
                    if (live) {
                        ls = s_ls[j]; le = s_le[j]; rs = s_rs[j]; re = s_re[j];
                        gp = s_gap[j]; th = s_thr[j]; sq = s_seq[j];
                    }
                    // ordered prefix of `live` over the workgroup
                    const unsigned long long lm = __ballot(live);
                    if (lane == 0) s_wcnt[tid >> 6] = (uint32_t)__popcll(lm);
                    __syncthreads();
                    uint32_t before = 0, tot = 0;
                    for (int wv = 0; wv < NW; ++wv) {
                        const uint32_t v = s_wcnt[wv];
                        if (wv < (tid >> 6)) before += v;
                        tot += v;
                    }
                    if (j < H) s_seq[j] = kNoSeq;  // every slot of this stripe has been read
                    __syncthreads();
                    if (live) {
                        const uint32_t d = w + before + (uint32_t)__popcll(lm & lt_mask);
                        s_ls[d] = ls; s_le[d] = le; s_rs[d] = rs; s_re[d] = re;
                        s_gap[d] = (SmallT)gp; s_thr[d] = th; s_seq[d] = sq; s_pend[d] = 0;
                    }
                    w += tot;
                    __syncthreads();
                }
                H = A;
                n_free = 0;
            }
        };
        // the flush of src/automaton.rs:182-200: every arm inactive
        auto maybe_close = [&]() {
            if (fam_open && A == 0) {
                ++fam_seq;
                next_seq = 0;
                fam_open = false;
            }
        };
        auto advance_quiet = [&](uint32_t q) {
            quiet += q;
            if (A > 0) age_and_retire(q * step, false, 0, 0, 0, true);
            maybe_close();
            if (A == 0 && quiet >= rp.tstar) done = true;
        };

        for (uint32_t g = g0; g < sg.g_end && !done;) {
            // ---- stage a batch of up to 64 probes (every wave computes the same masks) ----
            PROF_START();
            if (tid == 0) heartbeat(P, g0, g);
            ProbeBatch bt = load_batch<kHitBatch>(P.p_filt, P.row_off, g, sg.g_end, lane);
            const bool first_from_global = bt.n == 0;
            if (first_from_global) {  // a single row larger than the staging buffer: a batch of that one hit-probe, read where it is
                bt.n = 1;
                bt.hm = 1ull;
            }
            const unsigned long long base = bt.base;
            if (!first_from_global) {
                for (uint32_t r = tid; r < bt.tot; r += NT) s_hits[r] = P.hits[base + r];
            }
            __syncthreads();
            PROF_STOP(0);
            PROF_COUNT(1, 1);
            uint32_t pos = 0;
            while (!done) {
                uint32_t q;
                const uint32_t b = next_hit(bt, pos, q);
                if (q) {  // (behind the last hit-probe: the quiet probes that close the batch)
                    advance_quiet(q);
                    if (done) break;
                }
                if (b >= 64u) break;
                quiet = 0;
                pos = b + 1;
                const uint32_t cnt = lane_of(bt.f_l, b);
                const uint32_t off = lane_of(bt.rel_l, b);
                const uint64_t i = (uint64_t)(g + b - sg.pb + 1) * step;
                const unsigned long long row = base + off;
                if (A + cnt > cap_eff) {
                    overflow = true;
                    done = true;
                    break;
                }
                const bool from_lds = !first_from_global;
                PROF_COUNT(5, 1);
                PROF_COUNT(10, A);
                PROF_COUNT(11, cnt);
                PROF_MAX(9, A + cnt);
                PROF_START();
                // ---- (0)+(1) candidate index over the live arms ------------------------------
                uint32_t hmask = 63u;
                while (hmask + 1u < HT && hmask + 1u < 2u * A) hmask = (hmask << 1) | 1u;
                for (uint32_t h = tid; h <= hmask; h += NT) s_head[h] = 0xFFFFFFFFu;
                if (tid == 0) s_nwide = 0;
                __syncthreads();
                for (uint32_t j0 = 0; j0 < H; j0 += NT) {
                    const uint32_t j = j0 + tid;
                    uint32_t sq = kNoSeq, th = 0;
                    PosT re = 0;
                    if (j < H && (sq = s_seq[j]) != kNoSeq) {
                        th = s_thr[j];
                        re = s_re[j];
                    }
                    const bool live = sq != kNoSeq;
                    if (live && th <= G) {
                        const uint32_t bkt = (uint32_t)((uint64_t)re >> bsh);
                        s_next[j] = (IdxT)atomicExch(&s_head[((bkt * 2654435761u) >> 12) & hmask], j);
                    }
                    // wide arms: one LDS atomic per wave, not per arm
                    const bool wide = live && th > G;
                    const unsigned long long wm = __ballot(wide);
                    if (wm) {
                        const int leader = __ffsll((long long)wm) - 1;
                        uint32_t wbase = 0;
                        if (lane == leader) wbase = atomicAdd(&s_nwide, (uint32_t)__popcll(wm));
                        wbase = __shfl(wbase, leader);
                        const uint32_t d = wbase + (uint32_t)__popcll(wm & lt_mask);
                        if (wide) {
                            if constexpr (PACKED_WIDE) {
                                const uint64_t wv = (uint64_t)th + k - 1u;
                                s_ivlo[d] = (PosT)(re - k + 1u);
                                s_ivw[d] = wv > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)wv;
                                s_wkey[d] = ((unsigned long long)sq << kSlotBits) | j;
                            } else {
                                s_widx[d] = (IdxT)j;
                            }
                        }
                    }
                }
                __syncthreads();
                PROF_STOP(2);
                PROF_START();
                const uint32_t n_wide = s_nwide;
                const uint32_t seq_base = next_seq;
                for (uint32_t t0 = 0; t0 < cnt; t0 += NT) {
                    const uint32_t ct = min((uint32_t)NT, cnt - t0);
                    if (t0) __syncthreads();
                    // ---- (2) narrow arms: one thread per hit, two buckets ----------------------
                    PosT hx = 0;
                    if ((uint32_t)tid < ct) {
                        hx = from_lds ? s_hits[off + t0 + tid] : P.hits[row + t0 + tid];
                        const uint64_t lo_re = (uint64_t)hx + 1u > (uint64_t)G ? (uint64_t)hx + 1u - G : 0u;
                        const uint32_t b0 = (uint32_t)(lo_re >> bsh);
                        const uint32_t b1 = (uint32_t)(((uint64_t)hx + k - 1u) >> bsh);
                        unsigned long long best = ~0ull;
                        for (uint32_t bkt = b0; bkt <= b1; ++bkt) {
                            uint32_t j = s_head[((bkt * 2654435761u) >> 12) & hmask];
                            while (j != 0xFFFFFFFFu && j != kEndIdx) {
                                if (arm_accepts<PosT>(hx, s_re[j], s_thr[j], k))
                                    best = min(best, ((unsigned long long)s_seq[j] << kSlotBits) | j);
                                j = s_next[j];
                            }
                        }
                        s_best[tid] = best;
                    }
                    __syncthreads();
                    PROF_STOP(4);
                    PROF_START();
                    // ---- wide arms: thread = (hit, part of the packed list), branch-free --------
                    if (n_wide) {
                        const uint32_t Hr = (ct + 63u) & ~63u;  // hits rounded up to waves
                        const uint32_t NP = NT / Hr;            // list parts
                        const uint32_t tl = (uint32_t)tid % Hr, part = (uint32_t)tid / Hr;
                        const bool valid = tl < ct && part < NP;
                        PosT x = 0;
                        if (valid) x = from_lds ? s_hits[off + t0 + tl] : P.hits[row + t0 + tl];
                        if (part < NP) {  // wave-uniform
                            const uint32_t j0 = (uint32_t)((uint64_t)n_wide * part / NP);
                            const uint32_t j1 = (uint32_t)((uint64_t)n_wide * (part + 1) / NP);
                            unsigned long long found = ~0ull;
                            // 8 independent LDS load chains in flight per thread (the scan is
                            // latency-bound otherwise), smallest accepting key wins
                            uint32_t j = j0;
                            if constexpr (PACKED_WIDE) {
                                for (; j + 8 <= j1; j += 8) {
                                    PosT lo8[8];
                                    uint32_t w8[8];
                                    unsigned long long k8[8];
#pragma unroll
                                    for (int u = 0; u < 8; ++u) {
                                        lo8[u] = s_ivlo[j + u];
                                        w8[u] = s_ivw[j + u];
                                        k8[u] = s_wkey[j + u];
                                    }
#pragma unroll
                                    for (int u = 0; u < 8; ++u)
                                        found = min(found, (uint64_t)(PosT)(x - lo8[u]) < w8[u] ? k8[u] : ~0ull);
                                }
                                for (; j < j1; ++j)
                                    found = min(found, (uint64_t)(PosT)(x - s_ivlo[j]) < s_ivw[j] ? s_wkey[j] : ~0ull);
                            } else {
                                for (; j + 8 <= j1; j += 8) {
                                    uint32_t sl8[8], th8[8], sq8[8];
                                    PosT re8[8];
#pragma unroll
                                    for (int u = 0; u < 8; ++u) sl8[u] = s_widx[j + u];
#pragma unroll
                                    for (int u = 0; u < 8; ++u) {
                                        re8[u] = s_re[sl8[u]];
                                        th8[u] = s_thr[sl8[u]];
                                        sq8[u] = s_seq[sl8[u]];
                                    }
#pragma unroll
                                    for (int u = 0; u < 8; ++u) {
                                        const unsigned long long key = ((unsigned long long)sq8[u] << kSlotBits) | sl8[u];
                                        found = min(found, arm_accepts<PosT>(x, re8[u], th8[u], k) ? key : ~0ull);
                                    }
                                }
                                for (; j < j1; ++j) {
                                    const uint32_t slot = s_widx[j];
                                    const unsigned long long key = ((unsigned long long)s_seq[slot] << kSlotBits) | slot;
                                    found = min(found, arm_accepts<PosT>(x, s_re[slot], s_thr[slot], k) ? key : ~0ull);
                                }
                            }
                            if (valid && found != ~0ull) atomicMin(&s_best[tl], found);
                        }
                        __syncthreads();
                    }
                    PROF_STOP(8);
                    PROF_START();
                    // ---- (3) ExtendArm / NewArm, one thread per hit -----------------------------
                    const bool mine = (uint32_t)tid < ct;
                    unsigned long long best = ~0ull;
                    if (mine) {
                        best = s_best[tid];
                        if (best != ~0ull) pend_max(s_pend, (uint32_t)(best & kSlotMask), t0 + tid + 1u);
                    }
                    // unmatched hits become arms
                    const bool is_new = mine && best == ~0ull;
                    // rank of this hit among the new arms, in hit order (= creation order): every
                    // wave recomputes the per-group counts from s_best (no barrier)
                    uint32_t before = 0, n_new = 0;
                    for (uint32_t c0 = 0; c0 < ct; c0 += 64) {
                        const uint32_t hidx = c0 + lane;
                        const bool un = hidx < ct && s_best[hidx] == ~0ull;
                        const unsigned long long nm = __ballot(un);
                        const uint32_t pc = (uint32_t)__popcll(nm);
                        if (c0 < ((uint32_t)tid & ~63u)) before += pc;
                        else if (c0 == ((uint32_t)tid & ~63u)) before += (uint32_t)__popcll(nm & lt_mask);
                        n_new += pc;
                    }
                    if (is_new) {
                        // reuse empty slots first (top of the stack), then grow the high-water mark
                        const uint32_t slot = before < n_free ? (uint32_t)s_free[n_free - 1u - before]
                                                              : H + (before - n_free);
                        s_ls[slot] = (PosT)i; s_le[slot] = (PosT)(i + k); s_rs[slot] = hx;
                        s_re[slot] = (PosT)(hx + k);
                        s_gap[slot] = 0;  // aged to `step` by this very probe in (4)
                        s_thr[slot] = thr0;
                        s_seq[slot] = next_seq + before;
                        s_pend[slot] = 0;
                    }
                    if (n_new <= n_free) {
                        n_free -= n_new;
                    } else {
                        H += n_new - n_free;
                        n_free = 0;
                    }
                    A += n_new;
                    next_seq += n_new;
                    __syncthreads();
                }
                (void)seq_base;
                PROF_STOP(6);
                PROF_START();
                // ---- (4) apply ExtendArm (last hit in SA order wins), age, retire -----------------
                age_and_retire(step, true, i, off, row, from_lds);
                fam_open = true;
                maybe_close();
                PROF_STOP(7);
            }
            __syncthreads();
            g += bt.n;
        }
        if (!done && sg.g_end < sg.chunk_end) {
            if (tid == 0) atomicAdd(&P.ctr[CT_RANOUT], 1ull);
        } else if (!overflow && fam_open) {
            emit_records(tid == 0, (PosT)0, (PosT)0, (PosT)0, (PosT)0, kTombstone);
        }
        if (overflow && tid == 0) {
            const unsigned long long at = atomicAdd(P.ovf_count, 1ull);
            if (P.ovf_list) P.ovf_list[at] = g0;
        }
        if (tid < 64) {
            PROF_FLUSH();
        }
        __syncthreads();
    }
    rec_flush(rec_alloc, P, lane);
    wg_busy(P);
}

}  // namespace asgart
