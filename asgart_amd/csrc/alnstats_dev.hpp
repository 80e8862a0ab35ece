// alnstats_dev.hpp -- what the counts of an alignment consist of (asgart_alignment_stats; align.stats_host is the readable
// statement): the kind of a mismatch, the pair of bytes a base of an `X` run stands for, and how the lanes of a wave that
// hold consecutive items of consecutive rows find the part of the wave that is their row's.
//
// The frame is the alignment's: A is the left arm as stored, B the right arm as lev_dev.hpp's RightArm walks it (reversed
// if flag bit 0 is set, then complemented if bit 1 is).  Run t of duplication (left, right, ll, rl) starts at the arm
// offsets i_t and j_t of paf_dev.hpp -- the exclusive sums I and J of run_on_left and run_on_right, counted from the
// row's first run -- and base v of it pairs a = text[left + i_t + v] with b = B(j_t + v).
#pragma once
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
}  // namespace asgart
