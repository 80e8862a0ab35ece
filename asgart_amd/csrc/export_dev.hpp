// export_dev.hpp -- what a result file consists of, unit by unit: the one statement of the three formats that both stages of
// export.hip run, the length stage with a sink that counts and the write stage with a sink that stores.
//
// A file is prefix, body, suffix; prefix and suffix are the caller's.  The body is a sequence of UNITS: family unit 0, the
// records of family 0, family unit 1, the records of family 1, ..., family unit F.  Unit u is family unit f where
// u == offs[f] + f, and otherwise record q = u - f - 1 of the family f it follows; there are n + F + 1 units.
//   JSON (serde_json::to_string_pretty of RunResult.families, src/exporters.rs:12-25): family unit f closes family f - 1
//     (`\n    ]` unless it was empty), separates (`,\n`) and opens family f (`    [\n`, or the whole `    []` of an empty
//     one); unit 0 starts with the `[\n` of the array, unit F ends with its `\n  ]`; no family at all is `[]`.  A record is
//     the SD object at indent 6, led by `,\n` when it is not the first of its family.
//   GFF2 / GFF3 (GFF2Exporter::save :27-67, GFF3Exporter::save :69-113): a record is the two lines of its duplication,
//     family unit f >= 1 the empty line behind family f - 1 (`writeln!(out)`, :62 and :108), unit 0 nothing.
// A record is written in two HALVES, so that two threads can share it: the first ends behind chr_right_position (JSON) or
// behind the first line (GFF); a family unit is all first half.
#pragma once
#include "f32_digits.hpp"
#include "file_writer.hpp"

namespace asgart {

enum : int32_t { kFormatJson = 0, kFormatGff2 = 1, kFormatGff3 = 2 };

struct ExportIn : ResultView {   // (flags: bit 0 reversed, bit 1 complemented)
    const float *identity;     // [n], or nullptr: every identity 0
    const Pow10Entry *pow10;
    uint32_t n;
    int32_t format;
};

struct CountSink {
    uint64_t n = 0;
    __host__ __device__ void byte(uint8_t) { ++n; }
    template <size_t N>
    __host__ __device__ void lit(const char (&)[N]) { n += N - 1; }
    __host__ __device__ void zeros(uint32_t k) { n += k; }
    __host__ __device__ void bytes(const uint8_t *, uint64_t k) { n += k; }
    __host__ __device__ void u64(uint64_t v) {
        do {
            ++n;
            v /= 10;
        } while (v);
    }
};

struct ByteSink {
    uint8_t *p;
    __host__ __device__ void byte(uint8_t c) { *p++ = c; }
    template <size_t N>
    __host__ __device__ void lit(const char (&s)[N]) {
        for (size_t i = 0; i + 1 < N; ++i) p[i] = (uint8_t)s[i];
        p += N - 1;
    }
    __host__ __device__ void zeros(uint32_t k) {
        for (uint32_t i = 0; i < k; ++i) p[i] = '0';
        p += k;
    }
    __host__ __device__ void bytes(const uint8_t *src, uint64_t k) {
        for (uint64_t i = 0; i < k; ++i) p[i] = src[i];
        p += k;
    }
    __host__ __device__ void u64(uint64_t v) {
        uint32_t len = 0;
        for (uint64_t w = v; len == 0 || w; w /= 10) ++len;
        for (uint32_t i = len; i-- > 0; v /= 10) p[i] = (uint8_t)('0' + (uint32_t)(v % 10));
        p += len;
    }
};

struct Unit {
    uint32_t fam;     // the family unit's family, or the family of the record
    uint32_t rec;     // the record's ordinal among all duplications
    bool is_family;
};

// unit u of n + n_fam + 1: the largest f in [0, n_fam] with offs[f] + f <= u (offs[f] + f grows strictly)
__host__ __device__ inline Unit unit_of(const uint64_t *__restrict__ offs, uint32_t n_fam, uint32_t u) {
    uint32_t lo = 0, hi = n_fam + 1;   // the first f with offs[f] + f > u; offs[0] + 0 = 0 <= u
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offs[mid] + mid > u) hi = mid; else lo = mid + 1;
    }
    const uint32_t f = lo - 1;
    const bool fam = offs[f] + f == u;
    return Unit{f, fam ? 0u : u - f - 1, fam};
}

template <class Sink>
__host__ __device__ inline void emit_family_unit(Sink &s, const ExportIn &in, uint32_t f) {
    const uint32_t F = in.n_fam;
    if (in.format != kFormatJson) {
        if (f > 0) s.byte('\n');
        return;
    }
    if (F == 0) {
        s.lit("[]");
        return;
    }
    if (f == 0) s.lit("[\n");
    if (f > 0 && in.offs[f] > in.offs[f - 1]) s.lit("\n    ]");
    if (f > 0 && f < F) s.lit(",\n");
    if (f < F) {
        if (in.offs[f + 1] > in.offs[f]) s.lit("    [\n"); else s.lit("    []");
    } else {
        s.lit("\n  ]");
    }
}

template <class Sink>
__host__ __device__ inline void emit_name(Sink &s, const ExportIn &in, int32_t id) {
    const uint64_t a = in.name_off[id];
    s.bytes(in.names + a, in.name_off[id + 1] - a);
}

// The identity a record prints: GFF2 prints `sd.identity * 100.0`, one rounded f32 product (src/exporters.rs:44).
__host__ __device__ inline float export_identity(const ExportIn &in, uint32_t q) {
    const float v = in.identity ? in.identity[q] : 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    return in.format == kFormatGff2 ? __fmul_rn(v, 100.0f) : v;
#else
    return in.format == kFormatGff2 ? v * 100.0f : v;
#endif
}

// half 0 or 1 of record q, the j-th of family `fam`; d: the digits of export_identity(in, q)
template <class Sink>
__host__ __device__ inline void emit_record(Sink &s, const ExportIn &in, uint32_t q, uint32_t fam, uint32_t half,
                                            const F32Digits &d) {
    const uint64_t j = q - in.offs[fam];
    const uint8_t fl = in.flags[q];
    if (in.format == kFormatJson) {
        if (half == 0) {
            if (j) s.lit(",\n");
            s.lit("      {\n        \"chr_left\": ");
            emit_name(s, in, in.chr[2 * (size_t)q]);
            s.lit(",\n        \"chr_right\": ");
            emit_name(s, in, in.chr[2 * (size_t)q + 1]);
            s.lit(",\n        \"global_left_position\": ");
            s.u64(in.sds[4 * (size_t)q]);
            s.lit(",\n        \"global_right_position\": ");
            s.u64(in.sds[4 * (size_t)q + 1]);
            s.lit(",\n        \"chr_left_position\": ");
            s.u64(in.chr_pos[2 * (size_t)q]);
            s.lit(",\n        \"chr_right_position\": ");
            s.u64(in.chr_pos[2 * (size_t)q + 1]);
        } else {
            s.lit(",\n        \"left_length\": ");
            s.u64(in.sds[4 * (size_t)q + 2]);
            s.lit(",\n        \"right_length\": ");
            s.u64(in.sds[4 * (size_t)q + 3]);
            s.lit(",\n        \"left_seq\": null,\n        \"right_seq\": null,\n        \"identity\": ");
            render_f32(s, d, true);
            s.lit(",\n        \"reversed\": ");
            if (fl & 1) s.lit("true"); else s.lit("false");
            s.lit(",\n        \"complemented\": ");
            if (fl & 2) s.lit("true"); else s.lit("false");
            s.lit("\n      }");
        }
        return;
    }
    // one GFF line: the arm `half` (0 left, 1 right); every sum wraps as the u64 sums of the host exporters do
    const int32_t name = in.chr[2 * (size_t)q + half];
    const uint64_t one = in.format == kFormatGff3 ? 1 : 0;
    const uint64_t start = in.chr_pos[2 * (size_t)q + half] + one;
    const uint64_t end = start + in.sds[4 * (size_t)q + 2 + half];
    const bool minus = half == 1 && (fl & 1);
    emit_name(s, in, name);
    s.lit("\tASGART\tSD\t");
    s.u64(start);
    s.byte('\t');
    s.u64(end);
    if (in.format == kFormatGff2) {
        s.lit("\t#");
        render_f32(s, d, false);
        if (half == 0) s.lit("\t+\t.\tSD#"); else if (minus) s.lit("\t#-\t.\tSD#"); else s.lit("\t#+\t.\tSD#");
        s.u64(fam);
        s.byte('/');
        s.u64(j);
        s.byte('-');
        emit_name(s, in, name);
        s.byte('\n');
    } else {
        s.byte('\t');
        render_f32(s, d, false);
        if (minus) s.lit("\t-\t.\tID=SD#"); else s.lit("\t+\t.\tID=SD#");
        s.u64(fam);
        s.byte('-');
        s.u64(j);
        if (half == 1) {
            s.lit("-right;Parent=SD#");
            s.u64(fam);
            s.byte('-');
            s.u64(j);
        }
        s.lit(";Name=SD#");
        s.u64(fam);
        s.byte('-');
        s.u64(j);
        s.byte('\n');
    }
}

// The scratch slot the length stage leaves for the write stage: x the unit's family, y the identity's digits, z the rest
// of F32Digits and the kind of unit, w the record's ordinal among the duplications.
__host__ __device__ inline uint32_t pack_slot_meta(const F32Digits &d, bool is_family) {
    return d.nd | (uint32_t)(d.kk + 128) << 4 | d.cls << 12 | d.neg << 14 | (is_family ? 1u : 0u) << 15;
}
__host__ __device__ inline F32Digits unpack_slot_digits(uint32_t digits, uint32_t meta) {
    return F32Digits{digits, meta & 15u, (int32_t)(meta >> 4 & 255u) - 128, meta >> 12 & 3u, meta >> 14 & 1u};
}
__host__ __device__ inline bool slot_is_family(uint32_t meta) { return (meta >> 15 & 1u) != 0; }

}  // namespace asgart
