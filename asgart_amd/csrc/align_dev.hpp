// align_dev.hpp -- the geometry of the alignment kernels (align.hip) and what host and device both compute from it: the
// lengths of the two arms in either range mode and the checkpoint layout of one duplication.  Bands and lanes hold the rows
// that the score kernels' do (kLevBand, kLevRows), and the systolic step is theirs, stated in lev_dev.hpp (lev_column).
//
// OUT OF SCOPE here (one wave walks every pair, so a megabase pair runs on one wave): a 16-wave band pipeline for the
// forward pass of long arms (levenshtein_long_kernel's shape in score.hip), and _shard / _multi variants of the entry point.
#pragma once

#include "lev_dev.hpp"

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

}  // namespace asgart
