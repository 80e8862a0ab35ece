// alnstats_dev.hpp -- what the counts of an alignment consist of (asgart_alignment_stats; align.stats_host is the readable
// statement): the kind of a mismatch, the pair of bytes a base of an `X` run stands for, and how the lanes of a wave that
// hold consecutive items of consecutive rows find the part of the wave that is their row's; and, at the end, the host half
// of the call's checks, which asgart_alignment_variants (variants.hip) makes in the same words.
//
// The frame is the alignment's: A is the left arm as stored, B the right arm as lev_dev.hpp's RightArm walks it (reversed
// if flag bit 0 is set, then complemented if bit 1 is).  Run t of duplication (left, right, ll, rl) starts at the arm
// offsets i_t and j_t of paf_dev.hpp -- the exclusive sums I and J of run_on_left and run_on_right, counted from the
// row's first run -- and base v of it pairs a = text[left + i_t + v] with b = B(j_t + v).
#pragma once
#include "index.hpp"
#include "tool_base.hpp"
#include "lev_dev.hpp"
#include "paf_dev.hpp"

namespace asgart {

struct AlnStatsIn {
    const uint64_t *sds;        // [n][4]: global left, global right, left_length, right_length
    const uint8_t *flags;       // [n]: bit 0 reversed, bit 1 complemented
    const uint8_t *status;      // [n]: 1 aligned; anything else: ten zeros, runs unread
    const uint64_t *run_off;    // [n + 1]
    const uint32_t *run_len;    // [n_runs]
    const uint8_t *run_op;      // [n_runs]
    const uint8_t *text;        // the index's normalised text
    uint64_t *I, *J, *X;        // [n_runs + 1]: the runs' `=XI` bases, `=XD` bases, `X` bases; exclusive sums of them
    uint64_t *bad;              // the lowest duplication that fails a check, as q << 2 | kPafBad..; all ones: none
    uint64_t *counts;           // [n][kAlnCounts]
    uint32_t n_sd;
    uint64_t n_runs;
};

// the fields of asgart_align_counts, in its order
enum : uint32_t {
    kAlnMatch = 0, kAlnMismatch, kAlnTransition, kAlnTransversion, kAlnInsRuns, kAlnInsBases, kAlnDelRuns, kAlnDelBases,
    kAlnLongestMatch, kAlnLongestGap, kAlnCounts
};

// 1 for a purine (a, g), 2 for a pyrimidine (c, t), 0 for every other byte; A-Z count as a-z
__host__ __device__ inline uint32_t base_class(uint32_t c) {
    c = lower_base((uint8_t)c);
    return c == 'a' || c == 'g' ? 1u : c == 'c' || c == 't' ? 2u : 0u;
}

// 1 a transition, 2 a transversion, 0 neither (an N, any other byte, equal bytes)
__host__ __device__ inline uint32_t mismatch_kind(uint32_t a, uint32_t b) {
    const uint32_t ca = base_class(a), cb = base_class(b);
    if (ca == 0 || cb == 0 || lower_base((uint8_t)a) == lower_base((uint8_t)b)) return 0;
    return ca == cb ? 1u : 2u;
}

// the duplication whose runs hold run t (t < run_off[n_sd]): duplications without runs are stepped over
__host__ __device__ inline uint32_t row_of_run(const uint64_t *__restrict__ run_off, uint64_t lo, uint64_t hi, uint64_t t) {
    return (uint32_t)(first_above(run_off, lo, hi, t) - 1);
}

// kind of base v of the `X` run t of duplication q
__device__ inline uint32_t kind_of_base(const AlnStatsIn &in, uint32_t q, uint64_t t, uint64_t v) {
    const uint64_t *sd = in.sds + 4 * (size_t)q;
    const uint64_t b0 = in.run_off[q];
    const uint64_t i = in.I[t] - in.I[b0] + v, j = in.J[t] - in.J[b0] + v;
    const RightArm B = right_arm(in.text + sd[1], (uint32_t)sd[3], in.flags[q]);
    return mismatch_kind(in.text[sd[0] + i], B.at((uint32_t)j));
}

// The lanes of a wave hold items of rows that never decrease from lane to lane (rosary.hip's scheme): a lane `opens` where
// its row differs from the lane's below (lane 0 always opens).  -> the lane behind the last one of the calling lane's row.
__device__ inline uint32_t row_end_lane(unsigned long long open_mask, uint32_t lane) {
    const unsigned long long above = lane == 63 ? 0ull : open_mask & (~0ull << (lane + 1));
    return above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;
}
// the lanes [lane, end) as a mask
__device__ inline unsigned long long lanes_from_to(uint32_t lane, uint32_t end) {
    return (end == 64 ? ~0ull : (1ull << end) - 1ull) & (~0ull << lane);
}
// Sum and maximum over the lanes [lane, end) of the calling lane's row: after the six steps the lane that opens a row
// holds its row's.  (Every lane of the wave calls them.)
__device__ inline uint64_t row_sum(uint64_t v, uint32_t lane, uint32_t end) {
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint64_t o = (uint64_t)__shfl_down((unsigned long long)v, off);
        if (lane + off < end) v += o;
    }
    return v;
}
__device__ inline uint32_t row_max(uint32_t v, uint32_t lane, uint32_t end) {
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_down(v, off);
        if (lane + off < end && o > v) v = o;
    }
    return v;
}

// ---- the host side of the checks, for every call that takes asgart_alignment_stats' arguments (alnstats.hip,
// variants.hip): the same refusals in the same words, under the caller's name ---------------------------------------------

// what is checked before anything is launched; `result` is where the call's answer goes (counts, a handle)
inline int32_t check_alignment_arguments(const char *who, const asgart_index *idx, const asgart_proto_sd *sds,
                                         const uint8_t *flags, const uint8_t *status, int64_t n_sd,
                                         const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op,
                                         const void *result) {
    if (!idx) {
        set_error("%s: bad argument (no index: the bases are its text's)", who);
        return ASGART_E_ARG;
    }
    if (n_sd < 0 || (n_sd && (!sds || !flags || !status || !run_offsets || !result))) {
        set_error("%s: bad argument", who);
        return ASGART_E_ARG;
    }
    if (n_sd >= (int64_t)1 << 31) {
        set_error("%s: 2^31 duplications and more are not supported", who);
        return ASGART_E_CAP;
    }
    if (n_sd == 0) return 0;
    const uint64_t n_runs = run_offsets[n_sd];
    if (n_runs >= (uint64_t)1 << 32) {
        set_error("%s: run_offsets end at %llu; 2^32 runs and more are not supported", who, (unsigned long long)n_runs);
        return ASGART_E_CAP;
    }
    RC_TRY(check_csr(who, "run_offsets", run_offsets, n_sd, (int64_t)n_runs, "the run count", "duplication"));
    if (n_runs && (!run_len || !run_op)) {
        set_error("%s: bad argument (%llu runs and no run_len or run_op)", who, (unsigned long long)n_runs);
        return ASGART_E_ARG;
    }
    const uint64_t n_text = (uint64_t)idx->n;
    for (int64_t q = 0; q < n_sd; ++q) {
        if (status[q] != 1) continue;
        if (flags[q] & ~3u) {
            set_error("%s: duplication %lld has flag byte %u (bit 0 reversed, bit 1 complemented)", who, (long long)q,
                      (unsigned)flags[q]);
            return ASGART_E_ARG;
        }
        const asgart_proto_sd &sd = sds[q];
        if (sd.left > n_text || sd.right > n_text || sd.left_length > n_text - sd.left || sd.right_length > n_text - sd.right) {
            set_error("%s: duplication %lld reaches past the end of the text", who, (long long)q);
            return ASGART_E_ARG;
        }
        if (arms_too_long(sd)) {   // (the right arm is walked with lev_dev.hpp's 32-bit offsets)
            set_error("%s: arms of 2^32 bases are not supported", who);
            return ASGART_E_CAP;
        }
    }
    return 0;
}

// the message for the word the device checks left behind (bad = q << 2 | kPafBad.., not all ones) -> ASGART_E_ARG
inline int32_t refuse_runs(const char *who, uint64_t bad, const asgart_proto_sd *sds, const uint64_t *run_offsets,
                           const uint32_t *run_len, const uint8_t *run_op) {
    const long long q = (long long)(bad >> 2);
    const uint64_t b = run_offsets[q], e = run_offsets[q + 1];
    if ((bad & 3) == kPafBadSums) {
        uint64_t i = 0, j = 0;
        for (uint64_t t = b; t < e; ++t) {
            i += run_on_left(run_op[t], run_len[t]);
            j += run_on_right(run_op[t], run_len[t]);
        }
        set_error("%s: the runs of duplication %lld consume %llu and %llu bases of arms of %llu and %llu", who, q,
                  (unsigned long long)i, (unsigned long long)j, (unsigned long long)sds[q].left_length,
                  (unsigned long long)sds[q].right_length);
    } else if ((bad & 3) == kPafBadLen) {
        set_error("%s: duplication %lld has a run_len of 0 (a run of no base)", who, q);
    } else {
        uint64_t t = b;
        while (t + 1 < e && run_op_known(run_op[t])) ++t;
        set_error("%s: duplication %lld has run_op %u: an operation is one of `=`, `X`, `I`, `D`", who, q,
                  (unsigned)run_op[t]);
    }
    return ASGART_E_ARG;
}
}  // namespace asgart
