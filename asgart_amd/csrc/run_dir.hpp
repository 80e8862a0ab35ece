// run_dir.hpp -- the run directory: the suffix-array interval of every REPEATED k-mer, one 64-byte bucket per lookup.
//
// keys (index.hpp) is sorted, so the occurrences of a k-mer are one run of equal key words.  The prefix table and the
// bisection behind it (search_dev.hpp: kmer_range) are sized for the average k-mer, which occurs once; the probes the
// position bits leave over are the repeated ones, whose prefix-table bucket holds hundreds of slots: a dozen dependent
// key loads, a walk and a second bisection for two numbers that depend on the index and k alone.  The directory holds
// them: one entry per run of at least T equal key words, in a hash table of 64-byte buckets of four entries.  A lookup
// reads ONE bucket.  A run that found its bucket full is not in the table, and a key that is not found takes the path
// through the prefix table: the directory only ever shortens a lookup, no result depends on what got in.
//
//   entry   16 bytes: the key word, then lo (first slot of the run) in the low 40 bits and the run's length in the
//           high 24 -- one layout for 32- and 64-bit slots.  A saturated length: the end is bisected from lo.
//   empty   key word of all ones (a key holds codes 1..5 in 3 bits per base and at most 63 bits: never all ones)
//   bucket  multiply-shift of a mixed key word: any bucket count below 2^32
#pragma once

#include "common.hpp"

namespace asgart {

constexpr uint64_t kRunDirEmpty = ~0ull;
constexpr int kRunDirWays = 4;                        // entries per bucket
constexpr uint64_t kRunDirBucketBytes = 64;
constexpr uint64_t kRunDirLoBits = 40, kRunDirLoMax = (1ull << kRunDirLoBits) - 1ull;
constexpr uint64_t kRunDirLenSat = (1ull << 24) - 1ull;  // "take the end by bisection from lo"
constexpr uint64_t kRunDirMaxBuckets = 0xFFFFFFFFull;

__host__ __device__ inline uint64_t run_dir_pack(uint64_t lo, uint64_t len) {
    return (lo & kRunDirLoMax) | ((len < kRunDirLenSat ? len : kRunDirLenSat) << kRunDirLoBits);
}
__host__ __device__ inline uint64_t run_dir_lo(uint64_t w) { return w & kRunDirLoMax; }
__host__ __device__ inline uint64_t run_dir_len(uint64_t w) { return w >> kRunDirLoBits; }  // kRunDirLenSat: saturated

__host__ __device__ inline uint32_t run_dir_bucket(uint64_t key, uint32_t n_buckets) {
    uint64_t h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    return (uint32_t)(((h >> 32) * (uint64_t)n_buckets) >> 32);
}

}  // namespace asgart
