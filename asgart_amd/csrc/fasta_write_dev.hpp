// fasta_write_dev.hpp -- what a written FASTA file consists of, byte by byte, and how a window of the file finds the records
// and the intervals that have a byte in it: the write stage of fasta_write.hip.  Plain functions of (window, thread), so that
// a host program can run them thread by thread (tools/fasta_write_hostcheck.hip); nothing here needs more than <cstdint>.
//
// The file (include/asgart_hip.h states it; asgart_amd/mask.py: fasta_text_host is the readable statement).  Record r is
//   HEADER `\n` BODY        HEADER = header r as given, BODY = its bases in lines of `width`, each line followed by `\n`
// and starts at rec_off[r] (the host's 64-bit sum of the sizes in front of it; rec_off[n_rec] is the size of the file).  The
// body of a record of len bases has len + ceil(len / width) bytes (width 0: len + 1, or 0 for an empty record); body offset o
// is a `\n` iff o mod (width + 1) == width or o is the body's last byte, and the base o - o / (width + 1) otherwise.
// A base at strand position x inside an interval is masked: fill 0 turns 'A'..'Z' into lower case and keeps every other
// byte, any other fill replaces the byte.
//
// A window is kWindow consecutive BYTES of the file (fasta_write.hip), so it starts on a 16-byte line of the file whatever
// the records hold.  fasta_window_find: the records of its first and last byte by bisection of rec_off, and the intervals
// that can reach a base of it by bisection of the interval list.  fasta_window_compose: thread t of n composes the bytes
// t, t + n, t + 2n, .. of the window, so neighbouring lanes write neighbouring bytes of the image and -- a window's bases
// being one contiguous piece of the strand per record -- read neighbouring bytes of the strand.  A thread's bytes ascend, so
// its record and its interval only ever move forward: each is bisected again only when the byte has left it, between the
// cursor and the window's last.  The division by width + 1 is taken once per record and thread at 64 bits (the line of the
// record's first body byte in the window); a byte is at most a window behind that line's start, which 32 bits divide.
// A header longer than the window is composed by the windows it spans, each its own part; a window inside one interval,
// one line or one header runs the same statements.
#pragma once

#include <cstdint>

namespace asgart {

struct FastaIn {
    const uint8_t *src;         // the raw strand
    const uint64_t *rec_start;  // [n_rec] strand coordinates
    const uint64_t *rec_len;    // [n_rec]
    const uint64_t *rec_off;    // [n_rec + 1] where a record starts in the file; the last entry is the file's size
    const uint8_t *headers;     // the bytes of all header lines
    const uint64_t *hdr_off;    // [n_rec + 1]
    const uint64_t *iv;         // [n_iv][2]: start, end; ascending and disjoint
    uint64_t n_iv;
    uint32_t n_rec;
    uint32_t width;             // bases per line; 0: one line per record
    uint32_t fill;              // 0: lower case; else the byte a masked base becomes
};

struct FastaWindow {
    uint32_t r0, r1;  // the records of the window's first and last byte
    uint64_t i0, i1;  // the intervals that can hold a base of the window: [i0, i1)
};

// bytes of a line with its `\n`; one line per record is a line no record fills
__host__ __device__ inline uint64_t fasta_line_bytes(uint32_t width) {
    return width ? (uint64_t)width + 1 : (uint64_t)1 << 63;
}

__host__ __device__ inline uint64_t fasta_body_bytes(uint64_t len, uint32_t width) {
    if (len == 0) return 0;
    return width ? len + (len - 1) / width + 1 : len + 1;
}

// the first index in [lo, hi) with a[stride * index + shift] above v; hi when there is none
__host__ __device__ inline uint64_t fasta_first_above(const uint64_t *__restrict__ a, uint64_t stride, uint64_t shift,
                                                      uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[stride * mid + shift] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// how many bases of record r lie in front of byte g of the file (rec_off[r] <= g)
__host__ __device__ inline uint64_t fasta_bases_before(const FastaIn &in, uint32_t r, uint64_t g) {
    const uint64_t p = g - in.rec_off[r], head = in.hdr_off[r + 1] - in.hdr_off[r] + 1, len = in.rec_len[r];
    if (p <= head) return 0;
    const uint64_t q = p - head;
    if (q >= fasta_body_bytes(len, in.width)) return len;
    return q - q / fasta_line_bytes(in.width);
}

// g0 < g1 <= the file's size; n_rec >= 1
__host__ __device__ inline FastaWindow fasta_window_find(const FastaIn &in, uint64_t g0, uint64_t g1) {
    FastaWindow w;
    w.r0 = (uint32_t)(fasta_first_above(in.rec_off, 1, 0, 0, in.n_rec, g0) - 1);   // (rec_off[0] = 0 <= g0)
    w.r1 = (uint32_t)(fasta_first_above(in.rec_off, 1, 0, w.r0, in.n_rec, g1 - 1) - 1);
    // every base of the window lies in [x_lo, x_hi): the records ascend and do not overlap
    const uint64_t x_lo = in.rec_start[w.r0] + fasta_bases_before(in, w.r0, g0);
    const uint64_t x_hi = in.rec_start[w.r1] + fasta_bases_before(in, w.r1, g1);
    w.i0 = x_lo ? fasta_first_above(in.iv, 2, 1, 0, in.n_iv, x_lo) : 0;            // the first end above x_lo
    w.i1 = x_hi ? fasta_first_above(in.iv, 2, 0, w.i0, in.n_iv, x_hi - 1) : w.i0;  // the first start at or above x_hi
    return w;
}

// thread `tid` of `n_threads` composes its bytes of the window [g0, g1) into img (img[0] is the file's byte g0)
__host__ __device__ inline void fasta_window_compose(const FastaIn &in, const FastaWindow &w, uint64_t g0, uint64_t g1,
                                                     uint32_t tid, uint32_t n_threads, uint8_t *img) {
    const uint64_t line = fasta_line_bytes(in.width), span = g1 - g0;
    uint32_t r = w.r0;
    bool loaded = false;
    uint64_t off = 0, next_off = 0, head = 0, h_at = 0, rs = 0, body = 0, anchor = 0, lines_before = 0;
    uint64_t j = w.i0;
    for (uint64_t o = g0 + tid; o < g1; o += n_threads) {
        if (!loaded || o >= next_off) {
            next_off = in.rec_off[r + 1];
            if (o >= next_off) {   // the byte is behind the cursor's record: the records between the cursor and the last
                r = (uint32_t)(fasta_first_above(in.rec_off, 1, 0, (uint64_t)r + 1, (uint64_t)w.r1 + 1, o) - 1);
                next_off = in.rec_off[r + 1];
            }
            off = in.rec_off[r];
            h_at = in.hdr_off[r];
            head = in.hdr_off[r + 1] - h_at;
            rs = in.rec_start[r];
            body = fasta_body_bytes(in.rec_len[r], in.width);
            // the line of the record's first body byte in the window
            const uint64_t b_at = off + head + 1, q_first = g0 > b_at ? g0 - b_at : 0;
            lines_before = q_first / line;
            anchor = lines_before * line;
            loaded = true;
        }
        const uint64_t p = o - off;
        uint8_t c;
        if (p < head) {
            c = in.headers[h_at + p];
        } else if (p == head) {
            c = '\n';
        } else {
            const uint64_t q = p - head - 1, rel = q - anchor;   // rel < line + span
            uint64_t d, m;
            if (line <= span) {   // (the same in every thread of the window)
                const uint32_t rel32 = (uint32_t)rel, line32 = (uint32_t)line, d32 = rel32 / line32;
                d = d32;
                m = rel32 - d32 * line32;
            } else {              // rel < 2 * line
                d = rel >= line ? 1 : 0;
                m = rel - (d ? line : 0);
            }
            if (m == line - 1 || q == body - 1) {
                c = '\n';
            } else {
                const uint64_t x = rs + (q - (lines_before + d));
                c = in.src[x];
                if (j < w.i1 && in.iv[2 * j + 1] <= x) j = fasta_first_above(in.iv, 2, 1, j + 1, w.i1, x);
                if (j < w.i1 && in.iv[2 * j] <= x) {
                    if (in.fill)
                        c = (uint8_t)in.fill;
                    else if (c >= 'A' && c <= 'Z')
                        c |= 0x20;
                }
            }
        }
        img[o - g0] = c;
    }
}

}  // namespace asgart
