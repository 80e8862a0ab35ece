// paf_dev.hpp -- what a PAF file consists of, byte by byte: the one statement of a row's head that both stages of paf.hip
// run (the length stage with export_dev.hpp's CountSink, the write stage with a sink that stores the bytes inside a window of
// the file), and how a window of the file finds the rows and the runs that have a byte in it.
//
// A row (align.paf_text) is HEAD, CIGAR, `\n`.  The head is the twelve columns and the tags up to and including `cg:Z:`; the
// CIGAR is the text of the row's runs, `<length><operation>` each, in the order of the runs for a `+` row and in the reverse
// order for a `-` row.  With P the exclusive sum of the runs' text lengths, run t of a row whose runs are [b, e) starts
//   P[t] - P[b]        bytes into the CIGAR of a `+` row,
//   P[e] - P[t + 1]    bytes into the CIGAR of a `-` row: a suffix sum, so the reversal needs no pass of its own.
// Only the duplications with a row (status != 0) are numbered: row k is duplication kept[k], and row_start[k] grows strictly.
#pragma once
#include "export_dev.hpp"

namespace asgart {

struct PafIn {
    const uint64_t *offs;       // [n_fam + 1]
    const uint64_t *sds;        // [n][4]: global left, global right, left_length, right_length
    const uint8_t *flags;       // [n]: 0 `+`, 3 `-`
    const uint32_t *distance;   // [n]
    const int32_t *chr;         // [n][2] name ids
    const uint64_t *chr_pos;    // [n][2]
    const uint64_t *run_off;    // [n + 1]
    const uint32_t *run_len;    // [n_runs]
    const uint8_t *run_op;      // [n_runs]
    const uint8_t *names;       // the bytes of all names
    const uint64_t *name_off;   // [n_names + 1]
    const uint64_t *name_len;   // [n_names]: the length of the fragment, column 2 and 7
    const uint32_t *kept;       // [n_rows]: the duplications with a row, ascending
    const uint64_t *P, *M, *B;  // [n_runs + 1]: exclusive sums over the runs of text bytes, `=` bases, all bases
    const uint32_t *head_len;   // [n_rows]
    const uint32_t *fam;        // [n_rows]
    const uint64_t *row_start;  // [n_rows + 1]; the last entry is the size of the file
    uint32_t n_fam, n_rows;
};

// ByteSink for a window [g0, g1) of the file whose image starts at img: a byte outside the window is counted and dropped.
struct WindowSink {
    uint8_t *img;
    uint64_t at, g0, g1;
    __host__ __device__ void byte(uint8_t c) {
        if (at >= g0 && at < g1) img[at - g0] = c;
        ++at;
    }
    template <size_t N>
    __host__ __device__ void lit(const char (&s)[N]) {
        for (size_t i = 0; i + 1 < N; ++i) byte((uint8_t)s[i]);
    }
    __host__ __device__ void bytes(const uint8_t *src, uint64_t k) {   // (a name longer than the window costs the window)
        const uint64_t lo = at > g0 ? at : g0, hi = at + k < g1 ? at + k : g1;
        for (uint64_t p = lo; p < hi; ++p) img[p - g0] = src[p - at];
        at += k;
    }
    __host__ __device__ void u64(uint64_t v) {
        uint32_t len = 0;
        for (uint64_t w = v; len == 0 || w; w /= 10) ++len;
        for (uint32_t i = len; i-- > 0; v /= 10) {
            const uint64_t p = at + i;
            if (p >= g0 && p < g1) img[p - g0] = (uint8_t)('0' + (uint32_t)(v % 10));
        }
        at += len;
    }
};

__host__ __device__ inline uint32_t decimal_digits(uint32_t v) {
    uint32_t len = 1;
    for (; v >= 10; v /= 10) ++len;
    return len;
}

// the first index in [lo, hi) whose entry is above v (at least v); hi when there is none
__host__ __device__ inline uint64_t first_above(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__host__ __device__ inline uint64_t first_at_least(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The head of the row of duplication q, of family fam: columns 1 to 12, NM:i:, fm:i: and the `cg:Z:` its CIGAR follows.
// (P, M and B are read, head_len / fam / row_start are not: the length stage runs this before they exist.)
template <class Sink>
__host__ __device__ inline void emit_paf_head(Sink &s, const PafIn &in, uint32_t q, uint32_t fam) {
    const uint64_t b = in.run_off[q], e = in.run_off[q + 1];
    for (uint32_t arm = 0; arm < 2; ++arm) {
        const int32_t id = in.chr[2 * (size_t)q + arm];
        const uint64_t a = in.name_off[id], pos = in.chr_pos[2 * (size_t)q + arm];
        s.bytes(in.names + a, in.name_off[id + 1] - a);
        s.byte('\t');
        s.u64(in.name_len[id]);
        s.byte('\t');
        s.u64(pos);
        s.byte('\t');
        s.u64(pos + in.sds[4 * (size_t)q + 2 + arm]);
        s.byte('\t');
        if (arm == 0) {
            s.byte(in.flags[q] == 3 ? '-' : '+');
            s.byte('\t');
        }
    }
    s.u64(in.M[e] - in.M[b]);
    s.byte('\t');
    s.u64(in.B[e] - in.B[b]);
    s.lit("\t255\tNM:i:");
    s.u64(in.distance[q]);
    s.lit("\tfm:i:");
    s.u64(fam);
    s.lit("\tcg:Z:");
}

struct RunRange {
    uint64_t t0, t1;
};

// the runs of row k with a byte in [g0, g1): in both orientations a range of consecutive runs
__host__ __device__ inline RunRange runs_in_window(const PafIn &in, uint32_t k, uint64_t g0, uint64_t g1) {
    const uint32_t q = in.kept[k];
    const uint64_t b = in.run_off[q], e = in.run_off[q + 1];
    const uint64_t c_at = in.row_start[k] + in.head_len[k], c_end = c_at + (in.P[e] - in.P[b]);
    const uint64_t lo = g0 > c_at ? g0 : c_at, hi = g1 < c_end ? g1 : c_end;
    if (hi <= lo) return RunRange{0, 0};
    // run t covers P[t] .. P[t + 1] of the row's span of P, counted from its start (`+`) or back from its end (`-`)
    const bool minus = in.flags[q] == 3;
    const uint64_t x = minus ? in.P[e] - (hi - c_at) : in.P[b] + (lo - c_at);
    const uint64_t y = minus ? in.P[e] - (lo - c_at) : in.P[b] + (hi - c_at);
    return RunRange{first_above(in.P, b, e + 1, x) - 1, first_at_least(in.P, b, e + 1, y)};
}

__host__ __device__ inline void write_run(const PafIn &in, uint32_t k, uint64_t t, uint64_t g0, uint64_t g1, uint8_t *img) {
    const uint32_t q = in.kept[k];
    const uint64_t b = in.run_off[q], e = in.run_off[q + 1];
    const uint64_t off = in.flags[q] == 3 ? in.P[e] - in.P[t + 1] : in.P[t] - in.P[b];
    WindowSink s{img, in.row_start[k] + in.head_len[k] + off, g0, g1};
    s.u64(in.run_len[t]);
    s.byte(in.run_op[t]);
}

// Thread tid of n_threads composes its share of the bytes [g0, g1) of the file, 0 <= g0 < g1 <= size, into img.  The heads
// and line ends of the rows k0 .. k1 that hold g0 and g1 - 1 are dealt out row by row; the runs with a byte in the window
// -- a part of row k0's, all of the rows' between, a part of row k1's -- run by run.  Every byte of the window is stored
// exactly once; no thread walks the runs of a row.
__host__ __device__ inline void paf_compose(const PafIn &in, uint64_t g0, uint64_t g1, uint32_t tid, uint32_t n_threads,
                                            uint8_t *img) {
    const uint64_t *rs = in.row_start;
    const uint32_t k0 = (uint32_t)(first_above(rs, 0, (uint64_t)in.n_rows + 1, g0) - 1);
    const uint32_t k1 = (uint32_t)(first_above(rs, k0, (uint64_t)in.n_rows + 1, g1 - 1) - 1);
    for (uint64_t k = (uint64_t)k0 + tid; k <= k1; k += n_threads) {
        if (rs[k] + in.head_len[k] > g0) {
            WindowSink s{img, rs[k], g0, g1};
            emit_paf_head(s, in, in.kept[k], in.fam[k]);
        }
        const uint64_t nl = rs[k + 1] - 1;
        if (nl >= g0 && nl < g1) img[nl - g0] = '\n';
    }
    const RunRange first = runs_in_window(in, k0, g0, g1);
    RunRange last{0, 0}, mid{0, 0};
    if (k1 > k0) {
        last = runs_in_window(in, k1, g0, g1);
        mid = RunRange{in.run_off[in.kept[k0] + 1], in.run_off[in.kept[k1]]};
    }
    const uint64_t n_first = first.t1 - first.t0, n_mid = mid.t1 - mid.t0, n_last = last.t1 - last.t0;
    for (uint64_t i = tid; i < n_first + n_mid + n_last; i += n_threads) {
        if (i < n_first) {
            write_run(in, k0, first.t0 + i, g0, g1, img);
        } else if (i < n_first + n_mid) {
            // the duplication of the run by bisection of the run offsets, its row by bisection of kept; a duplication
            // without a row that was given runs all the same has none
            const uint64_t t = mid.t0 + (i - n_first);
            const uint32_t q = (uint32_t)(first_above(in.run_off, (uint64_t)in.kept[k0] + 1, (uint64_t)in.kept[k1] + 1, t) - 1);
            uint32_t lo = k0 + 1, hi = k1;
            while (lo < hi) {
                const uint32_t m = (lo + hi) >> 1;
                if (in.kept[m] >= q) hi = m; else lo = m + 1;
            }
            if (lo < k1 && in.kept[lo] == q) write_run(in, lo, t, g0, g1, img);
        } else {
            write_run(in, k1, last.t0 + (i - n_first - n_mid), g0, g1, img);
        }
    }
}

}  // namespace asgart
