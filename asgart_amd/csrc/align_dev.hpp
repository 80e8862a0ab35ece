// align_dev.hpp -- the geometry of the alignment kernels (align.hip) and what host and device both compute from it: the
// lengths of the two arms in either range mode and the checkpoint layout of one duplication.  Bands and lanes hold the rows
// that the score kernels' do (kLevBand, kLevRows), and the systolic step is theirs, stated in lev_dev.hpp (lev_column).
//
// The corridor of asgart_align_duplications_banded is here too (BandedShape): which columns of every band are computed for
// a bound on the distance, and where that band's checkpoints lie.
//
// OUT OF SCOPE here (one wave walks every pair, so a megabase pair runs on one wave, inside its corridor or not): a 16-wave
// band pipeline for the forward pass of long arms (levenshtein_long_kernel's shape in score.hip), and _shard / _multi
// variants of the entry points.
#pragma once

#include "lev_dev.hpp"

#include <algorithm>

namespace asgart {

constexpr uint32_t kAlignTile = 256u;                  // W: columns between two column checkpoints = columns of one tile
constexpr uint32_t kAlignDirWords = kAlignTile * 64u;  // one u32 of 16 two-bit directions per lane and column: 64 KiB of LDS
static_assert(kLevRows == 16, "a u32 holds the two-bit directions of a lane's rows");

// operations of a run, as the traceback numbers them and lev_column<true> packs them: the two low values are the diagonal
// with its cost
enum : uint32_t { kOpMatch = 0, kOpMismatch = 1, kOpInsert = 2, kOpDelete = 3, kOpNone = 4 };
static_assert(kOpMatch == 0 && kOpMismatch == 1 && kOpInsert == 2 && kOpDelete == 3, "the codes lev_column<true> writes");

// Checkpoints of one duplication of n x m cells, in u32 words from its (16-byte aligned) base:
//   colck[c * rows_padded + i]  = D[i + 1][(c + 1) W]   c < n_ck = floor((m - 1) / W): the columns W, 2W, .. < m
//   rowck[b * (m + 1) + j]      = D[(b + 1) kLevBand][j]   b < n_bands - 1, j in 1..m (entry 0 is never read: it is the row)
// rowck starts behind colck.  4 (n_bands - 1)(m + 1) + 4 floor((m - 1) / W) n_bands kLevBand bytes.
struct AlignShape {
    uint64_t n, m, n_bands, n_ck, rows_padded;
    __host__ __device__ uint64_t col_words() const { return n_ck * rows_padded; }
    __host__ __device__ uint64_t row_words() const { return (n_bands - 1u) * (m + 1u); }
    __host__ __device__ uint64_t bytes() const { return 4u * (col_words() + row_words()); }
};

__host__ __device__ inline AlignShape align_shape(const asgart_proto_sd &sd, int inclusive) {
    AlignShape g;
    g.n = sd.left_length + (inclusive ? 1u : 0u);
    g.m = sd.right_length + (inclusive ? 1u : 0u);
    g.n_bands = g.n ? (g.n + kLevBand - 1u) / kLevBand : 1u;
    g.n_ck = g.m ? (g.m - 1u) / kAlignTile : 0u;
    g.rows_padded = g.n_bands * kLevBand;
    return g;
}

// ---- the corridor (include/asgart_hip.h states the rule and proves what rests on it) --------------------------------
// For a bound T >= |m - n| every path of cost <= T stays on the diagonals j - i in [kmin, kmax].  Band b (rows
// b kLevBand + 1 .. min((b + 1) kLevBand, n)) computes the columns lo(b) .. hi(b), the smallest rectangle that holds those
// diagonals of its rows, clipped to [1, m]; every cell outside the rectangles counts as kAlignBig.  A rectangle is at most
// wmax = min(m, kLevBand + kmax - kmin) columns wide, and every band gets checkpoints of that size, so that an offset is a
// product (u32 words from the duplication's 16-byte aligned base):
//   colck[(b ck_per_band + c) kLevBand + r] = D[b kLevBand + r + 1][(first_ck(b) + c) W]   for the multiples of W in
//                                             [lo(b), hi(b) - 1]; ck_per_band = ceil((wmax - 1) / W) holds them all
//   rowck[b row_stride + j - lo(b) + 1]     = D[(b + 1) kLevBand][j]   b < n_bands - 1, j in lo(b) .. hi(b); row_stride = wmax + 1
// rowck starts behind colck.  4 n_bands ck_per_band kLevBand + 4 (n_bands - 1)(wmax + 1) bytes; none for T < |m - n| (nothing
// is computed) and for an empty arm.
constexpr uint32_t kAlignBig = 1u << 30;      // more than any bound; kAlignBig + n + m stays below 2^32 (the entry point sees to it)
constexpr uint64_t kAlignBandedCap = 1u << 30;  // n + m and max_distance stay below this

struct BandedShape {
    uint64_t n, m, n_bands, ck_per_band, row_stride;
    int64_t kmin, kmax;
    int beyond;  // T < |m - n|: more than T edits without any work
    __host__ __device__ uint32_t lo(uint64_t b) const {
        const int64_t v = (int64_t)(b * kLevBand) + 1 + kmin;
        return v < 1 ? 1u : (uint32_t)v;
    }
    __host__ __device__ uint32_t hi(uint64_t b) const {
        const uint64_t end = (b + 1u) * kLevBand < n ? (b + 1u) * kLevBand : n;
        const int64_t v = (int64_t)end + kmax;
        return v > (int64_t)m ? (uint32_t)m : (uint32_t)v;
    }
    __host__ __device__ uint32_t first_ck(uint64_t b) const { return (lo(b) + kAlignTile - 1u) / kAlignTile; }
    __host__ __device__ uint64_t col_words() const { return n_bands * ck_per_band * kLevBand; }
    __host__ __device__ uint64_t row_words() const { return (n_bands - 1u) * row_stride; }
    __host__ __device__ uint64_t bytes() const { return 4u * (col_words() + row_words()); }
    // the cells of the rectangles: what the forward pass computes
    uint64_t cells() const {
        uint64_t c = 0;
        for (uint64_t b = 0; !beyond && m && b * kLevBand < n; ++b)
            c += (((b + 1u) * kLevBand < n ? (b + 1u) * kLevBand : n) - b * kLevBand) * (uint64_t)(hi(b) - lo(b) + 1u);
        return c;
    }
};

__host__ __device__ inline BandedShape banded_shape(const asgart_proto_sd &sd, int inclusive, uint32_t max_distance) {
    BandedShape c;
    c.n = sd.left_length + (inclusive ? 1u : 0u);
    c.m = sd.right_length + (inclusive ? 1u : 0u);
    const int64_t delta = (int64_t)c.m - (int64_t)c.n, gap = delta < 0 ? -delta : delta;
    c.beyond = (int64_t)max_distance < gap;
    const int64_t e = c.beyond ? 0 : ((int64_t)max_distance - gap) / 2;
    c.kmin = (delta < 0 ? delta : 0) - e;
    c.kmax = (delta > 0 ? delta : 0) + e;
    c.n_bands = c.n ? (c.n + kLevBand - 1u) / kLevBand : 1u;
    const uint64_t span = (uint64_t)(c.kmax - c.kmin), wmax = c.m < kLevBand + span ? c.m : kLevBand + span;
    const bool none = c.beyond || c.n == 0 || c.m == 0;
    c.ck_per_band = none ? 0u : (wmax - 1u + kAlignTile - 1u) / kAlignTile;
    c.row_stride = none ? 0u : wmax + 1u;
    return c;
}

// The bounds of the automatic mode (max_distance == NULL).  REASONED, NOT SWEPT: the first bound is the length difference,
// which every alignment pays, plus 1/64 of the longer arm (1.6 % edits: the young, highly identical copies the corridor is
// for are within it, in a corridor of 1.6 % of the matrix), and at least 64, below which a corridor is narrower than a
// lane's 64-column chunk and saves nothing more.  A duplication beyond its bound is aligned again within 4 times that: the
// rounds that failed then cost a third of the one that succeeds (1/4 + 1/16 + ..), and the bound that succeeds is less
// than 4 times what was needed; 1.6 % -> 6.25 % -> 25 % -> the whole matrix is at most four rounds for a long pair.  n + m
// ends the series: that corridor is the whole matrix.
constexpr uint64_t kAlignAutoFloor = 64, kAlignAutoShare = 64, kAlignAutoFactor = 4;

inline uint32_t align_auto_first(uint64_t n, uint64_t m) {
    const uint64_t longer = n > m ? n : m, gap = n > m ? n - m : m - n;
    const uint64_t t = gap + std::max<uint64_t>(kAlignAutoFloor, longer / kAlignAutoShare);
    return (uint32_t)std::min<uint64_t>(t, n + m);
}

inline uint32_t align_auto_next(uint32_t bound, uint64_t n, uint64_t m) {
    return (uint32_t)std::min<uint64_t>(kAlignAutoFactor * (uint64_t)bound, n + m);
}

}  // namespace asgart
