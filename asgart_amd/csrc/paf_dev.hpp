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
//
// The cs:Z: column (asgart_paf_records_cs; align.cs_text is the readable statement).  A row of that writer is the row above,
// byte for byte, with one more column before the `\n`: HEAD, CIGAR, `\tcs:Z:`, CS, `\n`.  CS is the concatenation of the
// texts of the row's runs in the order of the CIGAR (as given for `+`, reversed for `-`); C, the exclusive sum of the runs'
// cs text lengths, places them as P places the CIGAR's.  Run t of duplication (left, right, ll, rl), n bases long, starts at
// the arm offsets
//   i_t = the lengths of the runs [b, t) with operation `=`, `X` or `I`    (I[t] - I[b]: bases of the left arm, the query),
//   j_t = the lengths of the runs [b, t) with operation `=`, `X` or `D`    (J[t] - J[b]: bases of the right arm, the target)
// -- in the order the runs are GIVEN, whatever the strand -- and stands for the base positions v = 0 .. n - 1:
//   row   query byte Q(v)                              target byte T(v)
//   `+`   text[left + i_t + v]                         text[right + j_t + v]
//   `-`   comp(text[left + i_t + n - 1 - v])           text[right + rl - j_t - n + v]
// comp is lev_dev.hpp's complement_base (ACGT and acgt swap, every other byte is kept); low maps A..Z to a..z and keeps every
// other byte.  On a `-` row the string runs along the target's forward strand and the query is shown reverse-complemented,
// as minimap2 writes it.  The text of a run, in the short (cs_mode 1) and the long (2) form:
//   `=`   short: `:` and the decimal n.   long: `=` and T(0 .. n-1) as stored
//   `X`   for each v: `*`, low(T(v)), low(Q(v))
//   `I`   `+` and low(Q(0 .. n-1))       (a left-arm base without a partner)
//   `D`   `-` and low(T(0 .. n-1))
// The writer prints what the runs say and compares no bases: an `X` over equal bytes prints two equal letters.
#pragma once
#include "export_dev.hpp"
#include "lev_dev.hpp"

namespace asgart {

struct PafIn : ResultView {     // (flags: 0 `+`, 3 `-`)
    const uint32_t *distance;   // [n]
    const uint64_t *run_off;    // [n + 1]
    const uint32_t *run_len;    // [n_runs]
    const uint8_t *run_op;      // [n_runs]
    const uint64_t *name_len;   // [n_names]: the length of the fragment, column 2 and 7
    const uint32_t *kept;       // [n_rows]: the duplications with a row, ascending
    const uint64_t *P, *M, *B;  // [n_runs + 1]: exclusive sums over the runs of text bytes, `=` bases, all bases
    const uint32_t *head_len;   // [n_rows]
    const uint32_t *fam;        // [n_rows]
    const uint64_t *row_start;  // [n_rows + 1]; the last entry is the size of the file
    uint32_t n_rows;
    // the cs:Z: column only (asgart_paf_records_cs):
    const uint8_t *text;        // the index's normalised text
    const uint64_t *C, *I, *J;  // [n_runs + 1]: exclusive sums over the runs of cs text bytes, `=XI` bases, `=XD` bases
    uint64_t *bad;              // the lowest row that fails a check, as row << 2 | kPafBad..; all ones: none
    uint32_t cs_mode;           // 1 short, 2 long
};

constexpr uint32_t kCsTagBytes = 6;   // `\tcs:Z:`
constexpr uint64_t kPafBadOp = 0, kPafBadLen = 1, kPafBadSums = 2;   // the checks of the cs writer, by rank within a row

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

// The two parts of a row that are made of runs: the exclusive sums that place a run's text in the part, and where the part
// of row k starts in the file.
struct CigarPart {
    __host__ __device__ static const uint64_t *sums(const PafIn &in) { return in.P; }
    __host__ __device__ static uint64_t at(const PafIn &in, uint32_t k) { return in.row_start[k] + in.head_len[k]; }
};
struct CsPart {
    __host__ __device__ static const uint64_t *sums(const PafIn &in) { return in.C; }
    __host__ __device__ static uint64_t at(const PafIn &in, uint32_t k) {
        const uint32_t q = in.kept[k];
        return in.row_start[k] + in.head_len[k] + (in.P[in.run_off[q + 1]] - in.P[in.run_off[q]]) + kCsTagBytes;
    }
};

// the runs of row k with a byte of the part in [g0, g1): in both orientations a range of consecutive runs
template <class Part>
__host__ __device__ inline RunRange runs_in_window(const PafIn &in, uint32_t k, uint64_t g0, uint64_t g1) {
    const uint64_t *S = Part::sums(in);
    const uint32_t q = in.kept[k];
    const uint64_t b = in.run_off[q], e = in.run_off[q + 1];
    const uint64_t c_at = Part::at(in, k), c_end = c_at + (S[e] - S[b]);
    const uint64_t lo = g0 > c_at ? g0 : c_at, hi = g1 < c_end ? g1 : c_end;
    if (hi <= lo) return RunRange{0, 0};
    // run t covers S[t] .. S[t + 1] of the row's span of S, counted from its start (`+`) or back from its end (`-`)
    const bool minus = in.flags[q] == 3;
    const uint64_t x = minus ? S[e] - (hi - c_at) : S[b] + (lo - c_at);
    const uint64_t y = minus ? S[e] - (lo - c_at) : S[b] + (hi - c_at);
    return RunRange{first_above(S, b, e + 1, x) - 1, first_at_least(S, b, e + 1, y)};
}

// where the text of run t of row k starts in the file
template <class Part>
__host__ __device__ inline uint64_t run_at(const PafIn &in, uint32_t k, uint64_t t) {
    const uint64_t *S = Part::sums(in);
    const uint32_t q = in.kept[k];
    const uint64_t b = in.run_off[q], e = in.run_off[q + 1];
    return Part::at(in, k) + (in.flags[q] == 3 ? S[e] - S[t + 1] : S[t] - S[b]);
}

__host__ __device__ inline void write_run(const PafIn &in, uint32_t k, uint64_t t, uint64_t g0, uint64_t g1, uint8_t *img) {
    WindowSink s{img, run_at<CigarPart>(in, k, t), g0, g1};
    s.u64(in.run_len[t]);
    s.byte(in.run_op[t]);
}

struct RowRange {
    uint32_t k0, k1;
};

// the rows that hold the bytes g0 and g1 - 1 of the file
__host__ __device__ inline RowRange rows_in_window(const PafIn &in, uint64_t g0, uint64_t g1) {
    const uint32_t k0 = (uint32_t)(first_above(in.row_start, 0, (uint64_t)in.n_rows + 1, g0) - 1);
    return RowRange{k0, (uint32_t)(first_above(in.row_start, k0, (uint64_t)in.n_rows + 1, g1 - 1) - 1)};
}

// The runs with a byte of the part in the window -- a part of row k0's, all of the rows' between, a part of row k1's -- dealt
// out run by run: thread tid of n_threads calls run(k, t) for its share of them.  No thread walks the runs of a row.
template <class Part, class Fn>
__host__ __device__ inline void deal_runs(const PafIn &in, RowRange r, uint64_t g0, uint64_t g1, uint32_t tid, uint32_t n_threads,
                                          Fn run) {
    const uint32_t k0 = r.k0, k1 = r.k1;
    const RunRange first = runs_in_window<Part>(in, k0, g0, g1);
    RunRange last{0, 0}, mid{0, 0};
    if (k1 > k0) {
        last = runs_in_window<Part>(in, k1, g0, g1);
        mid = RunRange{in.run_off[in.kept[k0] + 1], in.run_off[in.kept[k1]]};
    }
    const uint64_t n_first = first.t1 - first.t0, n_mid = mid.t1 - mid.t0, n_last = last.t1 - last.t0;
    for (uint64_t i = tid; i < n_first + n_mid + n_last; i += n_threads) {
        if (i < n_first) {
            run(k0, first.t0 + i);
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
            if (lo < k1 && in.kept[lo] == q) run(lo, t);
        } else {
            run(k1, last.t0 + (i - n_first - n_mid));
        }
    }
}

// Thread tid of n_threads composes its share of the bytes [g0, g1) of the file, 0 <= g0 < g1 <= size, into img: the heads
// and line ends of the rows that hold g0 and g1 - 1 and of those between, dealt out row by row, and the CIGAR runs with a
// byte in the window, run by run.  Every such byte of the window is stored exactly once.  kCs: the rows have the cs:Z: column;
// its tag is stored here with the head, its text is paf_cs_collect's and paf_cs_deal's.
template <bool kCs>
__host__ __device__ inline void paf_compose(const PafIn &in, uint64_t g0, uint64_t g1, uint32_t tid, uint32_t n_threads,
                                            uint8_t *img) {
    const uint64_t *rs = in.row_start;
    const RowRange r = rows_in_window(in, g0, g1);
    for (uint64_t k = (uint64_t)r.k0 + tid; k <= r.k1; k += n_threads) {
        if (rs[k] + in.head_len[k] > g0) {
            WindowSink s{img, rs[k], g0, g1};
            emit_paf_head(s, in, in.kept[k], in.fam[k]);
        }
        if constexpr (kCs) {
            WindowSink s{img, CsPart::at(in, (uint32_t)k) - kCsTagBytes, g0, g1};
            s.lit("\tcs:Z:");
        }
        const uint64_t nl = rs[k + 1] - 1;
        if (nl >= g0 && nl < g1) img[nl - g0] = '\n';
    }
    deal_runs<CigarPart>(in, r, g0, g1, tid, n_threads, [&](uint32_t k, uint64_t t) { write_run(in, k, t, g0, g1, img); });
}

// ---- the cs:Z: text ---------------------------------------------------------------------------------------------------

__host__ __device__ inline uint8_t lower_base(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c + ('a' - 'A')) : c; }

// A run as the arms see it (the cs writer's scans I and J, and alnstats.hip's): is its operation one of `=XID`, and the
// bases it consumes of the left and of the right arm.
__host__ __device__ inline bool run_op_known(uint8_t op) { return op == '=' || op == 'X' || op == 'I' || op == 'D'; }
__host__ __device__ inline uint64_t run_on_left(uint8_t op, uint32_t len) { return op != 'D' ? len : 0; }
__host__ __device__ inline uint64_t run_on_right(uint8_t op, uint32_t len) { return op != 'I' ? len : 0; }

// bytes of the cs text of a run of n bases (0 for an operation that is none: the row is refused before anything is written)
__host__ __device__ inline uint64_t cs_text_bytes(uint8_t op, uint32_t n, uint32_t cs_mode) {
    switch (op) {
    case '=': return cs_mode == 2 ? 1 + (uint64_t)n : 1 + decimal_digits(n);
    case 'X': return 3 * (uint64_t)n;
    case 'I':
    case 'D': return 1 + (uint64_t)n;
    default: return 0;
    }
}

// A run as the cs text sees it: where its text starts in the file, the text position of T(0), the text position of the
// byte behind Q(0) (Q walks up from it on a `+` row and down on a `-` row).  32 bytes: what the list of long runs holds.
struct CsRun {
    uint64_t at, tpos, qpos;
    uint32_t n;
    uint8_t op, minus;
};

__host__ __device__ inline CsRun cs_run(const PafIn &in, uint32_t k, uint64_t t) {
    const uint32_t q = in.kept[k];
    const uint64_t b = in.run_off[q];
    const uint64_t left = in.sds[4 * (size_t)q], right = in.sds[4 * (size_t)q + 1], rl = in.sds[4 * (size_t)q + 3];
    const uint64_t i = in.I[t] - in.I[b], j = in.J[t] - in.J[b];
    const uint32_t n = in.run_len[t];
    const bool minus = in.flags[q] == 3;
    // (an `I` run reads no target byte and a `D` run no query byte: their positions are never formed into an address)
    return CsRun{run_at<CsPart>(in, k, t), minus ? right + rl - j - n : right + j, minus ? left + i + n - 1 : left + i, n,
                 in.run_op[t], (uint8_t)minus};
}

// Byte o of the text of a run of any kind but the short `=` (cs_run_solo writes that one): the sign for o = 0 and one text
// byte otherwise for `I`, `D` and the long `=`; o mod 3 decides for `X`.  Lanes that take neighbouring o read neighbouring
// bytes of the text, ascending or (the query of a `-` row) descending; no alignment of either arm is assumed.
__host__ __device__ inline uint8_t cs_byte(const uint8_t *__restrict__ text, const CsRun &r, uint64_t o) {
    if (r.op == 'X') {
        const uint64_t v = o / 3;
        const uint32_t phase = (uint32_t)(o - 3 * v);
        if (phase == 0) return '*';
        if (phase == 1) return lower_base(text[r.tpos + v]);
        return lower_base(r.minus ? (uint8_t)complement_base(text[r.qpos - v]) : text[r.qpos + v]);
    }
    if (o == 0) return r.op == 'I' ? '+' : r.op == 'D' ? '-' : '=';
    const uint64_t v = o - 1;
    if (r.op == 'I') return lower_base(r.minus ? (uint8_t)complement_base(text[r.qpos - v]) : text[r.qpos + v]);
    const uint8_t c = text[r.tpos + v];
    return r.op == 'D' ? lower_base(c) : c;
}

// the bytes [lo, hi) of the file -- the text of r as far as it lies inside the window [g0, g1) -- by the calling thread alone
__host__ __device__ inline void cs_run_solo(const PafIn &in, const CsRun &r, uint64_t lo, uint64_t hi, uint64_t g0, uint64_t g1,
                                   uint8_t *img) {
    if (r.op == '=' && in.cs_mode != 2) {
        WindowSink s{img, r.at, g0, g1};
        s.byte(':');
        s.u64(r.n);
        return;
    }
    for (uint64_t p = lo; p < hi; ++p) img[p - g0] = cs_byte(in.text, r, p - r.at);
}

// The cs text inside the window [g0, g1), into img, by all n_threads threads of a workgroup, in two steps with a barrier
// between them (tid is the caller's; list and n_list are the workgroup's, *n_list == 0 behind a barrier before the first).
// paf_cs_collect: the runs with a byte in the window are dealt out a run per thread, as the CIGAR's are; a thread composes a
// run whose text inside the window is at most kSolo bytes (11 at least: the short `=`), and puts a longer one on the list.
// paf_cs_deal: the list is walked by every thread, and the bytes of each of its runs are dealt out by position across all of
// them: a window that lies wholly inside one run is composed by the whole workgroup.  The texts of the listed runs are
// disjoint parts of the window of more than kSolo bytes each, so (bytes of a window) / (kSolo + 1) entries hold them.
template <uint32_t kSolo, uint32_t kListMax>
__host__ __device__ inline void paf_cs_collect(const PafIn &in, uint64_t g0, uint64_t g1, uint32_t tid, uint32_t n_threads,
                                               uint8_t *img, CsRun *list, uint32_t *n_list) {
    deal_runs<CsPart>(in, rows_in_window(in, g0, g1), g0, g1, tid, n_threads, [&](uint32_t k, uint64_t t) {
        const CsRun r = cs_run(in, k, t);
        const uint64_t end = r.at + (in.C[t + 1] - in.C[t]);
        const uint64_t lo = r.at > g0 ? r.at : g0, hi = end < g1 ? end : g1;
        if (hi <= lo) return;
        if (hi - lo <= kSolo) {
            cs_run_solo(in, r, lo, hi, g0, g1, img);
            return;
        }
#ifdef __HIP_DEVICE_COMPILE__
        const uint32_t slot = atomicAdd(n_list, 1u);
#else
        const uint32_t slot = (*n_list)++;   // (a host harness runs the threads one behind the other)
#endif
        if (slot < kListMax) list[slot] = r;
    });
}

template <uint32_t kListMax>
__host__ __device__ inline void paf_cs_deal(const PafIn &in, uint64_t g0, uint64_t g1, uint32_t tid, uint32_t n_threads,
                                            uint8_t *img, const CsRun *list, const uint32_t *n_list) {
    const uint32_t n_long = *n_list < kListMax ? *n_list : kListMax;
    for (uint32_t l = 0; l < n_long; ++l) {
        const CsRun r = list[l];
        const uint64_t end = r.at + cs_text_bytes(r.op, r.n, 2);   // (a listed `=` is a long-form one)
        const uint64_t lo = r.at > g0 ? r.at : g0, hi = end < g1 ? end : g1;
        for (uint64_t p = lo + tid; p < hi; p += n_threads) img[p - g0] = cs_byte(in.text, r, p - r.at);
    }
}

}  // namespace asgart

