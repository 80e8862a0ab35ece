// variants_dev.hpp -- what a variant between the two arms of a duplication consists of (asgart_alignment_variants;
// align.variants_host is the readable statement), what an entry of a site is (asgart_variant_sites; align.sites_host), and
// the two handles that keep them on the device for the calls that follow (variants.hip makes them, variants_write.hip
// reads them).  include/asgart_hip.h states the rule; the frame, the arm offsets i_t and j_t and the checks of the runs
// are alnstats_dev.hpp's and paf_dev.hpp's.
#pragma once
#include "alnstats_dev.hpp"

// The records of one asgart_alignment_variants call, on the device of its index.
struct asgart_variants {
    int32_t device = 0;
    asgart::DevBuf records;                // asgart_variant[n_variants]
    std::vector<uint64_t> var_offsets;     // [n_sd + 1]: the records of duplication q; a copy the writers check rows by
    uint64_t n_variants = 0, n_snv = 0;
    double ms[3] = {0, 0, 0};
    ~asgart_variants() {
        if (records.p && hipSetDevice(device) == hipSuccess) records.release();
    }
};

// The sites of one asgart_variant_sites call, on the device of the records they were made from.
struct asgart_sites {
    int32_t device = 0;
    asgart::DevBuf pos, pairs, sd, ref, alt_mask, side;   // u64, u32, u32, u8, u8, u8 [n_sites]
    std::vector<uint64_t> var_offsets;                    // the records' (see above)
    uint64_t n_sites = 0, n_entries = 0;
    double ms[3] = {0, 0, 0};
    ~asgart_sites() {
        if (hipSetDevice(device) != hipSuccess) return;
        for (asgart::DevBuf *b : {&pos, &pairs, &sd, &ref, &alt_mask, &side})
            if (b->p) b->release();
    }
};

namespace asgart {

static_assert(sizeof(asgart_variant) == 32, "a record goes out as two 16-byte stores");

// what one run adds to the three sums the runs are scanned by, in one scan: its bases of the left and of the right arm
// (paf_dev.hpp's I and J) and its records (the bases of an `X` run, 1 for an `I` or a `D` run, 0 for `=`)
struct RunSums {
    uint64_t i, j, v;
};
struct RunSumsPlus {
    __host__ __device__ RunSums operator()(const RunSums &a, const RunSums &b) const {
        return RunSums{a.i + b.i, a.j + b.j, a.v + b.v};
    }
};
__host__ __device__ inline uint64_t run_records(uint8_t op, uint32_t len) {
    return op == 'X' ? len : (op == 'I' || op == 'D') ? 1u : 0u;
}

struct VariantsIn {
    const uint64_t *sds;        // [n][4]: global left, global right, left_length, right_length
    const uint8_t *flags;       // [n]: bit 0 reversed, bit 1 complemented
    const uint8_t *status;      // [n]: 1 aligned; anything else: no records, runs unread
    const uint64_t *run_off;    // [n + 1]
    const uint32_t *run_len;    // [n_runs]
    const uint8_t *run_op;      // [n_runs]
    const uint8_t *text;        // the index's normalised text
    RunSums *S;                 // [n_runs + 1]: what the runs add, then the exclusive sums of it
    uint64_t *bad;              // the lowest duplication that fails a check, as q << 2 | kPafBad..; all ones: none
    uint64_t *var_off;          // [n + 1]: S[run_off[q]].v
    uint32_t n_sd;
    uint64_t n_runs;
};

// the first run in [lo, hi) with more than k records in front of its end, that is S[t].v > k; hi when there is none
__host__ __device__ inline uint64_t first_records_above(const RunSums *__restrict__ S, uint64_t lo, uint64_t hi, uint64_t k) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (S[mid].v > k) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Record v of run t of duplication q (v = 0 for an `I` or a `D` run): the table of include/asgart_hip.h.  An `X` record
// reads one byte of either arm, inside the arms: the sums of the runs were checked against the arm lengths before.
__device__ inline asgart_variant variant_of(const VariantsIn &in, uint32_t q, uint64_t t, uint64_t v) {
    const uint64_t *sd = in.sds + 4 * (size_t)q;
    const uint64_t left = sd[0], right = sd[1], rl = sd[3];
    const uint64_t b0 = in.run_off[q];
    const uint64_t i = in.S[t].i - in.S[b0].i, j = in.S[t].j - in.S[b0].j;
    const uint8_t op = in.run_op[t], flag = in.flags[q];
    const bool rev = flag & 1;
    const uint32_t n = in.run_len[t];
    asgart_variant r;
    r.sd = q;
    r.op = op;
    r.flag = flag;
    r.left_base = r.right_base = 0;
    if (op == 'X') {
        r.left_pos = left + i + v;
        r.right_pos = right + (rev ? rl - 1 - (j + v) : j + v);
        r.left_len = r.right_len = 1;
        r.left_base = in.text[r.left_pos];
        r.right_base = in.text[r.right_pos];
    } else if (op == 'I') {
        r.left_pos = left + i;
        r.right_pos = right + (rev ? rl - j : j);
        r.left_len = n;
        r.right_len = 0;
    } else {
        r.left_pos = left + i;
        r.right_pos = right + (rev ? rl - j - n : j);
        r.left_len = 0;
        r.right_len = n;
    }
    return r;
}

// ---- sites ------------------------------------------------------------------------------------------------------------

// the class of a byte: 0 A, 1 C, 2 G, 3 T with the case folded, 4 (N) for every other byte
__host__ __device__ inline uint32_t site_class(uint32_t c) {
    switch (lower_base((uint8_t)c)) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
    default: return 4;
    }
}

// the letter a file prints for a class
__host__ __device__ inline uint8_t class_letter(uint32_t c) {
    return c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : c == 3 ? 'T' : 'N';
}

// Entry `side` (0 left, 1 right) of the `X` record r: the position, the class of the text's byte there and the class of the
// other arm's byte as this strand reads it (complemented when bit 1 of the record's flag is set).
struct SiteEntry {
    uint64_t pos;
    uint32_t ref, alt;
};
__host__ __device__ inline SiteEntry site_entry(const asgart_variant &r, uint32_t side) {
    const uint32_t mine = side ? r.right_base : r.left_base, other = side ? r.left_base : r.right_base;
    return SiteEntry{side ? r.right_pos : r.left_pos, site_class(mine),
                     site_class((r.flag & 2) ? complement_base(other) : other)};
}
// which of its two entries a record has, as bits 0 and 1: none for an indel, and none where the classes agree
__host__ __device__ inline uint32_t site_entries(const asgart_variant &r) {
    if (r.op != 'X') return 0;
    const SiteEntry l = site_entry(r, 0), g = site_entry(r, 1);
    return (l.ref != l.alt ? 1u : 0u) | (g.ref != g.alt ? 2u : 0u);
}

// OR over the lanes [lane, end) of the calling lane's row (alnstats_dev.hpp: row_sum's scheme)
__device__ inline uint32_t row_or(uint32_t v, uint32_t lane, uint32_t end) {
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_down(v, off);
        if (lane + off < end) v |= o;
    }
    return v;
}

}  // namespace asgart
