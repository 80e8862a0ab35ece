// lev_dev.hpp -- what the unit-cost edit-distance walks of score.hip and align.hip share, stated once: the geometry, the
// right arm as the walk reads it, the identity, the host's checks of a duplication list, and the straight-line pieces of
// one systolic step.  The step helpers serve align_forward_kernel and the tile rebuild of align_traceback_kernel;
// score.hip's two kernels run the same step from their own text (its header says why).
//
// One wave walks a band of 64 lanes x kLevRows rows.  Lane l owns kLevRows consecutive rows of the matrix (bases of the left
// arm) in registers and works on column s - l + 1 at step s, one column behind lane l-1; the value above the lane's first
// row and the column's base travel down the lanes, so a step is two cross-lane moves and 64 x kLevRows cells.
//
// Every site keeps its own loops over bands and steps, its own registers and its own fetch of the 64-column chunks of the
// top boundary and of the right arm (score.hip says why the loops are not shared); what is here is what a step does
// between those: lev_inputs, the site's column guard, lev_column, the site's extra, lev_store_bottom.
#pragma once

#include "common.hpp"

namespace asgart {

constexpr int kLevRows = 16;                    // rows per lane
constexpr uint32_t kLevBand = 64u * kLevRows;   // rows of one band (a wave's 64 lanes)

// utils::complement_nucleotide / structs::TR on the normalised alphabet; anything else is kept
__host__ __device__ inline uint32_t complement_base(uint32_t c) {
    switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'G': return 'C';
    case 'C': return 'G';
    case 'a': return 't';
    case 't': return 'a';
    case 'g': return 'c';
    case 'c': return 'g';
    default: return c;
    }
}

// the right arm as the DP walks it: reversed first, then complemented (src/structs.rs:443-448)
struct RightArm {
    const uint8_t *B;
    uint32_t lb;
    int reversed, complemented;
    __device__ uint32_t at(uint32_t j) const {
        const uint32_t c = B[reversed ? lb - 1u - j : j];
        return complemented ? complement_base(c) : c;
    }
};

// The orientation of duplication `item`: its flag byte (bit 0 reversed, bit 1 complemented, the encoding of
// asgart_extract_sequences) or, without a flag array, the call's two constants.  `item` is the same in every lane of
// the wave that picked the duplication up, so the byte is read once and kept in a scalar register.
__device__ inline uint32_t orientation_of(const uint8_t *flags, uint32_t item, int reversed, int complemented) {
    const uint32_t f = flags ? (uint32_t)flags[item] : (reversed ? 1u : 0u) | (complemented ? 2u : 0u);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)f);
}

__device__ inline RightArm right_arm(const uint8_t *B, uint32_t lb, uint32_t orient) {
    return RightArm{B, lb, (int)(orient & 1u), (int)(orient >> 1)};
}

__device__ inline float identity_of(const asgart_proto_sd &sd, uint32_t dist) {
    const uint64_t longest = sd.left_length > sd.right_length ? sd.left_length : sd.right_length;
    return (float)(100.0 * (1.0 - (double)dist / (double)longest));  // src/structs.rs:451, then `as f32`
}

// ---- one step of the walk, for the lane whose rows are i0+1 .. i0+kLevRows (1-based) ---------------------------------

// the lane's bases of the left arm; padding rows match nothing
__device__ __forceinline__ void lev_rows(uint32_t (&a)[kLevRows], uint32_t i0, uint32_t la, const uint8_t *A) {
#pragma unroll
    for (int r = 0; r < kLevRows; ++r) a[r] = i0 + r < la ? (uint32_t)A[i0 + r] : 0x100u;
}

// D[i][0] = i
__device__ __forceinline__ void lev_first_column(uint32_t (&col)[kLevRows], uint32_t i0) {
#pragma unroll
    for (int r = 0; r < kLevRows; ++r) col[r] = i0 + r + 1u;
}

struct LevIn {
    uint32_t up;  // D[i0][j], the value above the lane's first row
    uint32_t b;   // the base of column j
};

// What the lane's column of step s needs from outside: lane l-1 finished that column one step ago (last_out, b_pipe);
// lane 0 takes entry s & 63 of the two chunks the site fetched, 64 columns at a time.
__device__ __forceinline__ LevIn lev_inputs(uint32_t last_out, uint32_t top_chunk, uint32_t &b_pipe, uint32_t b_chunk,
                                            uint32_t s, int lane) {
    LevIn in;
    in.up = __shfl_up(last_out, 1);
    const uint32_t top0 = __shfl(top_chunk, (int)(s & 63u));
    in.b = __shfl_up(b_pipe, 1);
    const uint32_t b0 = __shfl(b_chunk, (int)(s & 63u));
    if (lane == 0) {
        in.up = top0;
        in.b = b0;
    }
    b_pipe = in.b;
    return in;
}

// The recurrence: col goes from column j-1 to column j, diag_in from D[i0][j-1] to D[i0][j].  With kDirs, also the
// direction of each of the rows, two bits each, as the traceback prefers them and as align_dev.hpp numbers them: the
// diagonal with its cost (kOpMatch 0, kOpMismatch 1), else up (kOpInsert 2), else left (kOpDelete 3).
template <bool kDirs>
__device__ __forceinline__ uint32_t lev_column(const uint32_t (&a)[kLevRows], uint32_t (&col)[kLevRows], uint32_t &diag_in,
                                               const LevIn &in) {
    uint32_t up = in.up, diag = diag_in, bits = 0;
#pragma unroll
    for (int r = 0; r < kLevRows; ++r) {
        const uint32_t left = col[r];
        const uint32_t cost = a[r] != in.b ? 1u : 0u;
        const uint32_t dg = diag + cost;
        const uint32_t v = min(dg, min(up, left) + 1u);
        if constexpr (kDirs) {
            // shifted in from the top, one v_alignbit_b32 a row: after the 16 rows, row r stands at bits 2r, 2r + 1
            static_assert(2 * kLevRows == 32, "the directions of a lane's rows fill a u32");
            const uint32_t d = v == dg ? cost : (v == up + 1u ? 2u : 3u);
            bits = __funnelshift_r(bits, d, 2);
        }
        diag = left;
        up = v;
        col[r] = v;
    }
    diag_in = in.up;
    return bits;
}

// D[la][j] out of the lane's column (the caller knows that row la is one of the lane's)
__device__ __forceinline__ uint32_t lev_row_value(const uint32_t (&col)[kLevRows], uint32_t i0, uint32_t la) {
    uint32_t v = 0;
#pragma unroll
    for (int r = 0; r < kLevRows; ++r)
        if (i0 + r + 1u == la) v = col[r];
    return v;
}

// The band's bottom row, the top boundary of the next band: lane 63 finishes column jo = s - 62 at step s; 64 of them are
// collected, one per lane, and stored together (bottom_row[1 .. lb]).
__device__ __forceinline__ void lev_store_bottom(uint32_t last_out, uint32_t s, int lane, uint32_t lb, uint32_t &out_chunk,
                                                 uint32_t *bottom_row) {
    const uint32_t v63 = __shfl(last_out, 63);
    const int64_t jo = (int64_t)s - 62;
    if (jo >= 1 && jo <= (int64_t)lb) {
        if ((uint32_t)lane == ((uint32_t)jo & 63u)) out_chunk = v63;
        if (((uint32_t)jo & 63u) == 63u || (uint32_t)jo == lb) {
            const uint32_t jw = ((uint32_t)jo & ~63u) + (uint32_t)lane;
            if (jw >= 1u && jw <= (uint32_t)jo) bottom_row[jw] = out_chunk;
        }
    }
}

// ---- the host's checks of a duplication list -------------------------------------------------------------------------

// the kernels count rows, columns and distances in 32 bits
inline bool arms_too_long(const asgart_proto_sd &sd) {
    return sd.left_length >= 0xFFFFFFFFull || sd.right_length >= 0xFFFFFFFFull ||
           sd.left_length + sd.right_length + 2u >= 0xFFFFFFFFull;
}

// A list of n_sd duplications and the array that receives one value for each: the pointers, then the count.  (Two
// functions: the sharded score calls report a bad shard count between the two, and asgart_compute_scores[_flags] has
// never looked at the count.)
inline int32_t check_list_pointers(const char *fn, const asgart_proto_sd *sds, int64_t n_sd, const void *out) {
    if (n_sd < 0 || (n_sd > 0 && (!sds || !out))) {
        set_error("%s: bad argument", fn);
        return ASGART_E_ARG;
    }
    return 0;
}

inline int32_t check_list_count(const char *fn, int64_t n_sd) {
    if ((uint64_t)n_sd >= 0xFFFFFFFFull) {  // (ordinals are 32-bit)
        set_error("%s: 2^32 duplications in one call are not supported", fn);
        return ASGART_E_CAP;
    }
    return 0;
}

inline int32_t check_list_args(const char *fn, const asgart_proto_sd *sds, int64_t n_sd, const void *out) {
    RC_TRY(check_list_pointers(fn, sds, n_sd, out));
    return check_list_count(fn, n_sd);
}

// one flag byte per duplication (NULL: none to check)
inline int32_t check_flags(const char *fn, const uint8_t *flags, int64_t n_sd) {
    for (int64_t q = 0; flags && q < n_sd; ++q)
        if (flags[q] & ~3u) {
            set_error("%s: duplication %lld has flag byte %u (bit 0 reversed, bit 1 complemented)", fn, (long long)q,
                      (unsigned)flags[q]);
            return ASGART_E_ARG;
        }
    return 0;
}

// The arms in the mode's own lengths: [p ..= p + len] with `inclusive` (the reference's slices, which panic past the end of
// the strand: src/structs.rs:441-442), [p .. p + len) without.
inline int32_t check_arms(const char *fn, uint64_t n_text, const asgart_proto_sd *sds, int64_t n_sd, int inclusive) {
    const uint64_t inc = inclusive ? 1u : 0u;
    for (int64_t q = 0; q < n_sd; ++q) {
        const asgart_proto_sd &sd = sds[q];
        if (sd.left > n_text || sd.right > n_text || sd.left_length + inc < inc || sd.right_length + inc < inc ||
            sd.left_length + inc > n_text - sd.left || sd.right_length + inc > n_text - sd.right) {
            set_error("%s: duplication %lld reaches past the end of the text", fn, (long long)q);
            return ASGART_E_ARG;
        }
        if (sd.left_length == 0 && sd.right_length == 0) {
            set_error("%s: duplication %lld has two empty arms", fn, (long long)q);
            return ASGART_E_ARG;
        }
        if (arms_too_long(sd)) {
            set_error("%s: arms of 2^32 bases are not supported", fn);
            return ASGART_E_CAP;
        }
    }
    return 0;
}

}  // namespace asgart
