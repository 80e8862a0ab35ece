// extend_wave_dev.hpp -- "K4", the extension kernel of tier 1: the seed-extension automaton, one wavefront per
// independent segment.
//
// Representation (equivalent to, not a transcription of, src/automaton.rs:87-200):
//   * only LIVE (active) arms are kept.  An arm that turns inactive can never
//     be extended again (try_extend_arms tests `a.active`, :68) and is only
//     looked at once more, when its family is flushed (:182-200), so it is
//     retired at once: written to the output list if len(right) >= M, dropped
//     otherwise.  (The reference's `retain` at :173-179 removes a subset of the
//     same arms; both removals are unobservable.)
//   * the family is flushed when the live list becomes empty; its members are
//     the retired arms, ordered by creation number (== position in the
//     reference's `arms` vector).  The host sorts records by
//     (segment start, family ordinal, creation number).
//   * arms still live at the end of the chunk are dropped AND their family's
//     retired members are void (:201-203): a tombstone record says so.
//   * <= 64 live arms: one arm per lane, in registers; otherwise LDS arrays.
//   * the hit rows of up to 64 consecutive probes are contiguous in the CSR and
//     are staged through LDS with one coalesced load.
#pragma once

#include "extend_common_dev.hpp"

namespace asgart {

constexpr uint32_t kEscalateCost = 40000;  // sum of (live arms + hits) over LDS-path probes

template <class PosT, int CAP>
__global__ __launch_bounds__(64) void extend_kernel(ExtParams<PosT> P) {
    __shared__ PosT s_ls[CAP], s_le[CAP], s_rs[CAP], s_re[CAP];
    __shared__ uint32_t s_gap[CAP], s_thr[CAP], s_seq[CAP], s_pend[CAP];
    __shared__ PosT s_hits[kHitBatch];
    // candidate index of the LDS path: arms bucketed by right end (see "LDS path")
    constexpr uint32_t HT = CAP <= 256 ? 256u : (CAP <= 1024 ? 1024u : 4096u);
    __shared__ uint32_t s_head[HT];
    __shared__ uint16_t s_next[CAP], s_wide[CAP];
    __shared__ PosT s_wlo[CAP];      // wide arms, packed: accepts x iff (x - s_wlo[w]) < s_ww[w]
    __shared__ uint32_t s_ww[CAP];
    const int lane = threadIdx.x;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const RunParams &rp = P.rp;
    const uint64_t n_seg = *P.n_seg_ptr;
    const uint32_t k = (uint32_t)rp.k, step = (uint32_t)rp.step, G = rp.G;
    const uint32_t thr0 = arm_threshold(k, G);
    RecAlloc rec_alloc;
    wg_begin(P);
    PROF_DECL;

    // Segments are fetched kFetch at a time (one contended global atomic per group).  The list is
    // sorted longest first: in its head the members of a group are strided, so that the longest
    // segments go to different waves instead of eight of them to the same one.
    constexpr unsigned long long kFetch = 8;
    const unsigned long long head_groups = min((unsigned long long)gridDim.x, n_seg / kFetch);
    const unsigned long long head = head_groups * kFetch;
    unsigned long long seg_base = 0;
    uint32_t seg_j = (uint32_t)kFetch;
    for (;;) {
        if (seg_j == (uint32_t)kFetch) {
            unsigned long long sb = 0;
            if (lane == 0) sb = atomicAdd(P.cursor, kFetch);
            seg_base = uni(sb);
            seg_j = 0;
        }
        const uint32_t j = seg_j++;
        const unsigned long long seg = seg_base < head ? seg_base / kFetch + (unsigned long long)j * head_groups
                                                       : seg_base + j;
        if (seg_base >= n_seg) break;
        if (seg >= n_seg) continue;
        const uint32_t g0 = P.seg_list[seg];
        PROF_SEG_BEGIN();
        if (lane == 0 && j == 0) {
            heartbeat(P, g0, 0u);
            seg_clock(P);
        }  // (once per fetched group of segments)
        const SegHeader sg = load_segment(rp, g0);

        // live arms: lane j holds arm j while in_regs (A <= 64), else s_*[0..A)
        PosT r_ls = 0, r_le = 0, r_rs = 0, r_re = 0;
        uint32_t r_gap = 0, r_thr = 0, r_seq = 0;
        uint32_t A = 0, quiet = 0, fam_seq = 0, next_seq = 0, lds_cost = 0;
        bool in_regs = true, overflow = false, done = false, fam_open = false;  // fam_open: a family is pending

        // ---- helpers -------------------------------------------------------
        auto emit_records = [&](bool emit, PosT ls, PosT le, PosT rs, PosT re, uint32_t seq) {
            const unsigned long long em = __ballot(emit);
            if (!em) return;
            const unsigned long long at = rec_slot(rec_alloc, P, em, lane);
            if (emit) write_record(P, at, g0, fam_seq, seq, 0u, sg.cs, sg.cl, sg.rev, ls, le, rs, re);
        };
        // the flush of src/automaton.rs:182-200: every arm inactive
        auto maybe_close = [&]() {
            if (fam_open && A == 0) {
                ++fam_seq;
                next_seq = 0;
                fam_open = false;
            }
        };
        // retire arms whose gap reached G (src/automaton.rs:166-171 + flush bookkeeping)
        auto retire_regs = [&]() {
            const bool dead = (uint32_t)lane < A && r_gap >= G;
            if (!__ballot(dead)) return;
            emit_records(dead && (uint64_t)(r_re - r_rs) >= rp.M, r_ls, r_le, r_rs, r_re, r_seq);
            const bool alive = (uint32_t)lane < A && !dead;
            const unsigned long long am = __ballot(alive);
            if (alive) {
                const int d = __popcll(am & lt_mask);
                s_ls[d] = r_ls; s_le[d] = r_le; s_rs[d] = r_rs; s_re[d] = r_re;
                s_gap[d] = r_gap; s_thr[d] = r_thr; s_seq[d] = r_seq;
            }
            __syncthreads();
            A = (uint32_t)__popcll(am);
            if ((uint32_t)lane < A) {
                r_ls = s_ls[lane]; r_le = s_le[lane]; r_rs = s_rs[lane]; r_re = s_re[lane];
                r_gap = s_gap[lane]; r_thr = s_thr[lane]; r_seq = s_seq[lane];
            }
            __syncthreads();
        };
        auto retire_lds = [&]() {
            uint32_t w = 0;
            bool any_dead = false;
            for (uint32_t t0 = 0; t0 < A; t0 += 64) {
                const uint32_t j = t0 + lane;
                PosT ls = 0, le = 0, rs = 0, re = 0;
                uint32_t gp = 0, th = 0, sq = 0;
                bool valid = j < A;
                if (valid) {
                    ls = s_ls[j]; le = s_le[j]; rs = s_rs[j]; re = s_re[j];
                    gp = s_gap[j]; th = s_thr[j]; sq = s_seq[j];
                }
                const bool dead = valid && gp >= G;
                any_dead |= __ballot(dead) != 0ull;
                emit_records(dead && (uint64_t)(re - rs) >= rp.M, ls, le, rs, re, sq);
                const bool alive = valid && !dead;
                const unsigned long long am = __ballot(alive);
                __syncthreads();
                if (alive && any_dead) {
                    const uint32_t d = w + __popcll(am & lt_mask);
                    s_ls[d] = ls; s_le[d] = le; s_rs[d] = rs; s_re[d] = re;
                    s_gap[d] = gp; s_thr[d] = th; s_seq[d] = sq; s_pend[d] = 0;
                }
                w += __popcll(am);
                __syncthreads();
            }
            A = w;
        };
        auto to_lds = [&]() {
            if ((uint32_t)lane < A) {
                s_ls[lane] = r_ls; s_le[lane] = r_le; s_rs[lane] = r_rs; s_re[lane] = r_re;
                s_gap[lane] = r_gap; s_thr[lane] = r_thr; s_seq[lane] = r_seq; s_pend[lane] = 0;
            }
            __syncthreads();
            in_regs = false;
        };
        auto to_regs = [&]() {
            if ((uint32_t)lane < A) {
                r_ls = s_ls[lane]; r_le = s_le[lane]; r_rs = s_rs[lane]; r_re = s_re[lane];
                r_gap = s_gap[lane]; r_thr = s_thr[lane]; r_seq = s_seq[lane];
            }
            __syncthreads();
            in_regs = true;
        };
        // q consecutive processed probes without hits
        auto advance_quiet = [&](uint32_t q) {
            quiet += q;
            if (A > 0) {
                const uint32_t add = q * step;
                if (in_regs) {
                    if ((uint32_t)lane < A) r_gap = r_gap + add < r_gap ? 0xFFFFFFFFu : r_gap + add;
                    retire_regs();
                } else {
                    for (uint32_t j = lane; j < A; j += 64) {
                        const uint32_t gp = s_gap[j];
                        s_gap[j] = gp + add < gp ? 0xFFFFFFFFu : gp + add;
                    }
                    __syncthreads();
                    PROF_STOP(7);
                    PROF_START();
                    retire_lds();
                    if (A <= 32) to_regs();
                    PROF_STOP(8);
                }
            }
            maybe_close();
            if (A == 0 && quiet >= rp.tstar) done = true;
        };

        for (uint32_t g = g0; g < sg.g_end && !done;) {
            // ---- stage a batch of up to 64 probes ------------------------------
            PROF_START();
            ProbeBatch bt = load_batch<kHitBatch>(P.p_filt, P.row_off, g, sg.g_end, lane);
            const bool first_from_global = bt.n == 0;
            if (first_from_global) {  // a single row larger than the staging buffer: a batch of that one hit-probe, read where it is
                bt.n = 1;
                bt.hm = 1ull;
            }
            const unsigned long long base = bt.base;
            if (!first_from_global) {
                const uint32_t tot = bt.tot;
                // four loads per lane in flight per round trip; most batches need a single round
                for (uint32_t r0 = 0; r0 < tot; r0 += 256u) {
                    PosT tmp[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t r = r0 + lane + 64u * u;
                        tmp[u] = r < tot ? P.hits[base + r] : (PosT)0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t r = r0 + lane + 64u * u;
                        if (r < tot) s_hits[r] = tmp[u];
                    }
                }
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
                if (in_regs && A + cnt <= 64u && !first_from_global) {
                    // ---------------- register path -------------------------------
                    PROF_START();
                    PROF_COUNT(3, 1);
                    PROF_MAX(9, A + cnt);
                    bool pend = false;
                    PosT pend_x = 0;
                    uint32_t newc = 0;
                    for (uint32_t t = 0; t < cnt; ++t) {
                        const PosT x = s_hits[off + t];
                        const bool ok = (uint32_t)lane < A && arm_accepts<PosT>(x, r_re, r_thr, k);
                        const unsigned long long m = __ballot(ok);
                        if (m) {  // ExtendArm on the first matching arm; last hit wins
                            if (lane == __ffsll((long long)m) - 1) {
                                pend = true;
                                pend_x = x;
                            }
                        } else {  // NewArm
                            if ((uint32_t)lane == A + newc) {
                                r_ls = (PosT)i; r_le = (PosT)(i + k); r_rs = x; r_re = (PosT)(x + k);
                                r_gap = step;  // not dirty: aged by this very probe
                                r_thr = thr0;
                                r_seq = next_seq + newc;
                            }
                            ++newc;
                        }
                    }
                    if ((uint32_t)lane < A) {
                        if (pend) {
                            r_re = (PosT)(pend_x + k);
                            r_le = (PosT)(i + k);
                            r_thr = arm_threshold((uint64_t)(i + k) - (uint64_t)r_ls, G);
                            r_gap = 0;
                        } else {
                            r_gap += step;
                        }
                    }
                    A += newc;
                    next_seq += newc;
                    retire_regs();
                    PROF_STOP(2);
                } else {
                    // ---------------- LDS path ------------------------------------
                    if (in_regs) to_lds();
                    // hand the segment to the block-cooperative heavy tier when it does not fit
                    // this wave's LDS share, or keeps producing many-hit x many-arm probes
                    lds_cost += A + cnt;
                    if (A + cnt > min((uint32_t)CAP, P.cap_limit) || lds_cost > P.escalate_cost) {
#ifdef ASGART_PROFILE_EXTEND
                        if (lane == 0) printf("[light overflow] g0=%u g=%u A=%u cnt=%u cost=%u first_glob=%d\n", g0, g + b, A, cnt, lds_cost, (int)first_from_global);
#endif
                        overflow = true;
                        done = true;
                        break;
                    }
                    const uint32_t A_old = A;
                    const bool from_lds = !first_from_global;
                    PROF_COUNT(5, 1);
                    PROF_COUNT(10, A_old);
                    PROF_COUNT(11, cnt);
                    PROF_MAX(9, A_old + cnt);
                    PROF_START();
                    // An arm accepts hit x iff  re - k < x < re + thr  (d_ss of src/automaton.rs:207-216
                    // with m = [x, x+k) and len(right) >= k).  So instead of testing every arm
                    // (automaton.rs:67-78) the arms whose thr is the floor G ("narrow") are hashed by
                    // bucket(re) with bucket width G + k: a hit can only be accepted by narrow arms
                    // in two buckets.  The few arms with a long left segment (thr > G) are kept in a
                    // list and tested one by one.  The answer is the smallest accepting arm index.
                    const uint32_t Wb = G + k;
                    uint32_t hmask = 63u;  // table sized to the live arms (power of two <= HT)
                    while (hmask + 1u < HT && hmask + 1u < 2u * A_old) hmask = (hmask << 1) | 1u;
                    for (uint32_t h = lane; h <= hmask; h += 64) s_head[h] = 0xFFFFFFFFu;
                    __syncthreads();
                    uint32_t n_wide = 0;
                    for (uint32_t t0 = 0; t0 < A_old; t0 += 64) {
                        const uint32_t j = t0 + lane;
                        const bool valid = j < A_old;
                        const bool narrow = valid && s_thr[j] <= G;
                        if (narrow) {
                            const uint32_t b = (uint32_t)((uint64_t)s_re[j] / Wb);
                            const uint32_t h = ((b * 2654435761u) >> 12) & hmask;
                            s_next[j] = (uint16_t)atomicExch(&s_head[h], j);
                        }
                        const unsigned long long wm = __ballot(valid && !narrow);
                        if (valid && !narrow) {
                            const uint32_t d = n_wide + __popcll(wm & lt_mask);
                            const uint32_t th = s_thr[j];
                            const uint64_t wv = (uint64_t)th + k - 1u;
                            s_wide[d] = (uint16_t)j;
                            s_wlo[d] = (PosT)(s_re[j] - k + 1u);
                            s_ww[d] = wv > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)wv;
                        }
                        n_wide += __popcll(wm);
                    }
                    __syncthreads();
                    PROF_STOP(4);
                    PROF_START();
                    for (uint32_t t0 = 0; t0 < cnt; t0 += 64) {
                        const uint32_t t = t0 + lane;
                        const bool valid = t < cnt;
                        PosT x = 0;
                        if (valid) x = from_lds ? s_hits[off + t] : P.hits[row + t];
                        uint32_t best = 0xFFFFFFFFu;
                        if (valid) {
                            // narrow candidates: re in (x - G, x + k)
                            const uint64_t lo_re = (uint64_t)x + 1u > (uint64_t)G ? (uint64_t)x + 1u - G : 0u;
                            const uint32_t b0 = (uint32_t)(lo_re / Wb);
                            const uint32_t b1 = (uint32_t)(((uint64_t)x + k - 1u) / Wb);
                            for (uint32_t b = b0; b <= b1; ++b) {
                                uint32_t j = s_head[((b * 2654435761u) >> 12) & hmask];
                                while (j != 0xFFFFFFFFu && j != 0xFFFFu) {
                                    if (j < best && arm_accepts<PosT>(x, s_re[j], s_thr[j], k)) best = j;
                                    j = s_next[j];
                                }
                            }
                        }
                        {   // wide arms: branch-free scan of the packed list (increasing arm index)
                            uint32_t wbest = 0xFFFFFFFFu;
                            uint32_t wdx = 0;
                            for (; wdx + 4 <= n_wide; wdx += 4) {
                                const uint32_t a0 = (uint64_t)(PosT)(x - s_wlo[wdx]) < s_ww[wdx] ? wdx : 0xFFFFFFFFu;
                                const uint32_t a1 = (uint64_t)(PosT)(x - s_wlo[wdx + 1]) < s_ww[wdx + 1] ? wdx + 1 : 0xFFFFFFFFu;
                                const uint32_t a2 = (uint64_t)(PosT)(x - s_wlo[wdx + 2]) < s_ww[wdx + 2] ? wdx + 2 : 0xFFFFFFFFu;
                                const uint32_t a3 = (uint64_t)(PosT)(x - s_wlo[wdx + 3]) < s_ww[wdx + 3] ? wdx + 3 : 0xFFFFFFFFu;
                                wbest = min(wbest, min(min(a0, a1), min(a2, a3)));
                            }
                            for (; wdx < n_wide; ++wdx)
                                wbest = min(wbest, (uint64_t)(PosT)(x - s_wlo[wdx]) < s_ww[wdx] ? wdx : 0xFFFFFFFFu);
                            if (valid && wbest != 0xFFFFFFFFu) best = min(best, (uint32_t)s_wide[wbest]);
                        }
                        const int found = best == 0xFFFFFFFFu ? -1 : (int)best;
                        if (valid && found >= 0) atomicMax(&s_pend[found], t + 1u);
                        const bool is_new = valid && found < 0;
                        const unsigned long long m = __ballot(is_new);
                        if (is_new) {
                            const uint32_t d = A + __popcll(m & lt_mask);
                            s_ls[d] = (PosT)i; s_le[d] = (PosT)(i + k); s_rs[d] = x;
                            s_re[d] = (PosT)(x + k);
                            s_gap[d] = step;
                            s_thr[d] = thr0;
                            s_seq[d] = next_seq + (d - A_old);
                            s_pend[d] = 0;
                        }
                        A += __popcll(m);
                    }
                    next_seq += A - A_old;
                    __syncthreads();
                    PROF_STOP(6);
                    PROF_START();
                    for (uint32_t j = lane; j < A_old; j += 64) {
                        const uint32_t pd = s_pend[j];
                        if (pd) {
                            s_pend[j] = 0;
                            const PosT x = from_lds ? s_hits[off + pd - 1u] : P.hits[row + pd - 1u];
                            s_re[j] = (PosT)(x + k);
                            s_le[j] = (PosT)(i + k);
                            s_thr[j] = arm_threshold((uint64_t)(i + k) - (uint64_t)s_ls[j], G);
                            s_gap[j] = 0;
                        } else {
                            s_gap[j] += step;
                        }
                    }
                    __syncthreads();
                    PROF_STOP(7);
                    PROF_START();
                    retire_lds();
                    if (A <= 32) to_regs();
                    PROF_STOP(8);
                }
                // every hit of this probe extended an arm or created one
                fam_open = true;
                maybe_close();
            }
            __syncthreads();
            g += bt.n;
        }
        // arms still alive at the end of the chunk are dropped together with the
        // unflushed family they belong to (src/automaton.rs:201-203)
        if (!done && sg.g_end < sg.chunk_end) {
            // sharded call: the segment is not finished inside the look-ahead window
            if (lane == 0) atomicAdd(&P.ctr[CT_RANOUT], 1ull);
        } else if (!overflow && fam_open)
            emit_records(lane == 0, (PosT)0, (PosT)0, (PosT)0, (PosT)0, kTombstone);
        PROF_FLUSH();
        if (overflow && lane == 0) {
            const unsigned long long at = atomicAdd(P.ovf_count, 1ull);
            if (P.ovf_list) P.ovf_list[at] = g0;
        }
        __syncthreads();
    }
    rec_flush(rec_alloc, P, lane);
    wg_busy(P);
}

}  // namespace asgart
