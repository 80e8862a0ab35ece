// chain_dev.hpp -- the link of the chaining rule (include/asgart_hip.h), the packed group key of the order and the wave
// primitives of the segment walk in chain.hip.  chain_link and ChainGroupKey are host and device code, for the stand-alone
// host checks of tools/.  chain_link: the rule's inequalities and t(j, i) in unsigned 64-bit arithmetic that
// cannot wrap for what the host has let through (position + length does not wrap, lengths are 1 .. 2^32 - 1,
// max_gap < 2^62).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace asgart {

constexpr uint32_t kChainLanes = 64;          // one wave walks a segment: the lanes of one window round
constexpr uint32_t kChainMaxLookback = 1024;  // the ring of a wave: 1024 scores of 8 bytes, 8 KiB of LDS
constexpr int64_t kNoScore = INT64_MIN;       // below every score: f and g are at least 1, f + t above -2^62

struct ChainAnchor {
    uint64_t pl, pr, ll, rl;
};

// Is there a link j -> i, and what is it worth?  j is given by its starts and ends.  The signed dl and dr of the rule are
// split into a gap and an overlap, of which at most one is above 0: the gap is compared with max_gap before anything is
// subtracted from it, and the overlap is below the length it is taken from (el_i > el_j gives el_j - pl_i < ll_i; on the
// right the same from the progress of the ends), so both new lengths are at least 1.
__host__ __device__ inline bool chain_link(uint64_t pl_j, uint64_t el_j, uint64_t pr_j, uint64_t er_j, const ChainAnchor &i,
                                           bool reversed, uint64_t max_gap, int64_t *t) {
    const uint64_t el_i = i.pl + i.ll, er_i = i.pr + i.rl;
    if (!(i.pl > pl_j && el_i > el_j)) return false;
    uint64_t gap_r, over_r;
    if (reversed) {
        if (!(i.pr < pr_j && er_i < er_j)) return false;
        gap_r = pr_j >= er_i ? pr_j - er_i : 0;
        over_r = er_i > pr_j ? er_i - pr_j : 0;
    } else {
        if (!(i.pr > pr_j && er_i > er_j)) return false;
        gap_r = i.pr >= er_j ? i.pr - er_j : 0;
        over_r = er_j > i.pr ? er_j - i.pr : 0;
    }
    const uint64_t gap_l = i.pl >= el_j ? i.pl - el_j : 0, over_l = el_j > i.pl ? el_j - i.pl : 0;
    if (gap_l > max_gap || gap_r > max_gap) return false;
    const uint64_t new_l = i.ll - over_l, new_r = i.rl - over_r;
    *t = (int64_t)(new_l < new_r ? new_l : new_r) - (int64_t)(gap_l > gap_r ? gap_l : gap_r);
    return true;
}

// The key of the third pass of the order, the group of duplication q: cl, cr (name_bits each, ids below 2^name_bits) and
// the two flag bits, 2 * name_bits + 2 bits in all; equal (cl, cr, fl) give equal keys, and the keys order as the triples do.
struct ChainGroupKey {
    const int32_t *__restrict__ chr;
    const uint8_t *__restrict__ flags;
    unsigned name_bits;
    __host__ __device__ uint64_t operator()(uint32_t q) const {
        return ((uint64_t)(uint32_t)chr[2 * (size_t)q] << (name_bits + 2)) | ((uint64_t)(uint32_t)chr[2 * (size_t)q + 1] << 2) |
               flags[q];
    }
};

#if defined(__HIPCC__)
__device__ inline int64_t wave_max(int64_t v) {
    for (int d = 32; d > 0; d >>= 1) {
        const int64_t o = (int64_t)__shfl_xor((long long)v, d);
        v = o > v ? o : v;
    }
    return v;
}

// the lowest lane whose flag is set (the caller knows there is one)
__device__ inline uint32_t first_lane(bool flag) { return (uint32_t)__ffsll((long long)__ballot(flag)) - 1u; }

__device__ inline uint64_t lane_value(uint64_t v, uint32_t lane) { return (uint64_t)__shfl((unsigned long long)v, (int)lane); }
__device__ inline int64_t lane_value(int64_t v, uint32_t lane) { return (int64_t)__shfl((long long)v, (int)lane); }
__device__ inline int32_t lane_value(int32_t v, uint32_t lane) { return __shfl(v, (int)lane); }

// the wave-wide shift of the register window: lane l takes lane l - 1's value, lane 0 takes `first`
__device__ inline uint64_t shift_in(uint64_t v, uint64_t first) {
    const uint64_t up = (uint64_t)__shfl_up((unsigned long long)v, 1);
    return threadIdx.x == 0 ? first : up;
}
__device__ inline int64_t shift_in(int64_t v, int64_t first) {
    const int64_t up = (int64_t)__shfl_up((long long)v, 1);
    return threadIdx.x == 0 ? first : up;
}
__device__ inline int32_t shift_in(int32_t v, int32_t first) {
    const int32_t up = __shfl_up(v, 1);
    return threadIdx.x == 0 ? first : up;
}
#endif

}  // namespace asgart
