// sdtable_dev.hpp -- what a row of the duplication table consists of, byte by byte: the one statement both stages of
// sdtable.hip run, the length stage with export_dev.hpp's CountSink and the write stage with its ByteSink.
//
// A file (align.sd_table_text) is the header line, which is the caller's prefix, and one row per duplication with a row
// (status != 0), in order; row k is duplication kept[k].  A row is 25 columns separated by tabs and ended by `\n`
// (include/asgart_hip.h names them), written in two HALVES so that two threads can share it: the first ends behind the
// family, column 11; the second is the counts, the four figures and the line end.  Apart from its two names a row is at
// most 4 * 20 + 12 + 10 + 10 * 20 + 4 * 49 + 31 = 529 bytes.
#pragma once
#include "export_dev.hpp"

namespace asgart {

struct SdTableIn : ResultView {   // (flags: 0 `+`, 3 `-`)
    const uint32_t *kept;      // [n_rows]: the duplications with a row, ascending
    const uint64_t *counts;    // [n][10]: asgart_align_counts
    const float *figures[4];   // [n] each: fracMatch, fracMatchIndel, jcK, k2K
    const Pow10Entry *pow10;
    uint32_t n_rows;
};

// half 0 or 1 of the row of duplication q, of family fam
template <class Sink>
__host__ __device__ inline void emit_sd_row(Sink &s, const SdTableIn &in, uint32_t q, uint32_t fam, uint32_t half) {
    if (half == 0) {
        for (uint32_t arm = 0; arm < 2; ++arm) {
            const int32_t id = in.chr[2 * (size_t)q + arm];
            const uint64_t a = in.name_off[id], pos = in.chr_pos[2 * (size_t)q + arm];
            s.bytes(in.names + a, in.name_off[id + 1] - a);
            s.byte('\t');
            s.u64(pos);
            s.byte('\t');
            s.u64(pos + in.sds[4 * (size_t)q + 2 + arm]);
            s.byte('\t');
        }
        s.lit("sd");
        s.u64(q);
        if (in.flags[q] == 3) s.lit("\t0\t+\t-\t"); else s.lit("\t0\t+\t+\t");
        s.u64(fam);
        return;
    }
    const uint64_t *c = in.counts + 10 * (size_t)q;
    const uint64_t match = c[0], mismatch = c[1], ins_runs = c[4], ins_bases = c[5], del_runs = c[6], del_bases = c[7];
    const uint64_t ints[10] = {match + mismatch + ins_bases + del_bases, match + mismatch, match, mismatch, c[2], c[3],
                               ins_runs + del_runs, ins_bases + del_bases, c[8], c[9]};
    for (uint32_t i = 0; i < 10; ++i) {
        s.byte('\t');
        s.u64(ints[i]);
    }
    for (uint32_t i = 0; i < 4; ++i) {
        s.byte('\t');
        render_f32(s, f32_shortest_digits(in.figures[i][q], in.pow10), false);
    }
    s.byte('\n');
}

}  // namespace asgart
