// align_dev.hpp -- the geometry of the alignment kernels (align.hip) and what host and device both compute from it: the
// lengths of the two arms in either range mode and the checkpoint layout of one duplication.
//
// OUT OF SCOPE here (one wave walks every pair, so a megabase pair runs on one wave): a 16-wave band pipeline for the
// forward pass of long arms (levenshtein_long_kernel's shape in score.hip), and _shard / _multi variants of the entry point.
#pragma once

#include "common.hpp"

namespace asgart {

constexpr int kAlignRows = 16;                         // rows per lane, as score.hip's kScoreRows
constexpr uint32_t kAlignBand = 64u * kAlignRows;      // rows of one band (a wave's 64 lanes)
constexpr uint32_t kAlignTile = 256u;                  // W: columns between two column checkpoints = columns of one tile
constexpr uint32_t kAlignDirWords = kAlignTile * 64u;  // one u32 of 16 two-bit directions per lane and column: 64 KiB of LDS

// operations of a run, as the traceback numbers them: the two low values are the diagonal with its cost
enum : uint32_t { kOpMatch = 0, kOpMismatch = 1, kOpInsert = 2, kOpDelete = 3, kOpNone = 4 };

// utils::complement_nucleotide on the normalised alphabet, as complement_base of score.hip: anything else is kept
__host__ __device__ inline uint32_t align_complement(uint32_t c) {
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

// Checkpoints of one duplication of n x m cells, in u32 words from its (16-byte aligned) base:
//   colck[c * rows_padded + i]  = D[i + 1][(c + 1) W]   c < n_ck = floor((m - 1) / W): the columns W, 2W, .. < m
//   rowck[b * (m + 1) + j]      = D[(b + 1) kAlignBand][j]   b < n_bands - 1, j in 1..m (entry 0 is never read: it is the row)
// rowck starts behind colck.  4 (n_bands - 1)(m + 1) + 4 floor((m - 1) / W) n_bands kAlignBand bytes.
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
    g.n_bands = g.n ? (g.n + kAlignBand - 1u) / kAlignBand : 1u;
    g.n_ck = g.m ? (g.m - 1u) / kAlignTile : 0u;
    g.rows_padded = g.n_bands * kAlignBand;
    return g;
}

}  // namespace asgart
