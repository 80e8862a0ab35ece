// result_read_dev.hpp -- what the device reader of result files (result_read.hip) accepts, stated once: the class byte of a
// byte of the file, the structural tokens between records and the pairs of them that may follow each other, and the walk over
// one record (the 13 fields of SD, reference src/structs.rs:471-495, as serde_json writes and reads them).  Whatever is not
// accepted here is refused with a rule; nothing is ever repaired or guessed.
#pragma once

#include "common.hpp"

namespace asgart {

// ---- the scan -------------------------------------------------------------------------------------------------------------
// The summary of a stretch of bytes for the backslash runs: bit 1 = all of it is backslashes, bit 0 = the parity of the run of
// backslashes it ends in.  Two stretches combine to the summary of both; associative, so a scan carries runs of any length.
struct BsOp {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return (b & 2u) ? ((a & 2u) | ((a ^ b) & 1u)) : b; }
};

__host__ __device__ inline bool is_ws(uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// the class byte: in a string (its two quotes included), a quote that delimits, and the nesting depth clamped to 0..15 -- of an
// opening bracket the depth it opens, of a closing one the depth it closes, of anything else the depth it lies in
constexpr uint32_t kClsString = 0x80, kClsQuote = 0x40, kClsDepth = 0x0F;

// the refusals of the parse
enum : uint32_t {
    kRuleStray = 1, kRuleStruct, kRuleKey, kRuleDup, kRuleMissing, kRuleColon, kRuleUint, kRuleBool, kRuleSeq, kRuleSeqNull,
    kRuleIdent, kRuleName, kRuleNest, kRuleComma, kRuleEnd
};

// ---- between the records --------------------------------------------------------------------------------------------------
// `families` opens depth 2, a family depth 3, a record depth 4.
enum : int {
    kTokAllOpen = 0, kTokAllClose, kTokFamOpen, kTokFamClose, kTokRecOpen, kTokRecClose, kTokCommaFam, kTokCommaRec,
    kStructNone = -1,   // whitespace, or the inside of a record: not this stage's
    kStructBad = -2     // a byte that has no place here
};

__device__ inline int struct_type(uint32_t c, uint32_t cl) {
    const uint32_t d = cl & kClsDepth;
    if (cl & kClsString) return d <= 3 ? kStructBad : kStructNone;
    if (is_ws(c)) return kStructNone;
    switch (d) {
    case 2: return c == '[' ? kTokAllOpen : c == ']' ? kTokAllClose : c == ',' ? kTokCommaFam : kStructBad;
    case 3: return c == '[' ? kTokFamOpen : c == ']' ? kTokFamClose : c == ',' ? kTokCommaRec : kStructBad;
    case 4: return c == '{' ? kTokRecOpen : c == '}' ? kTokRecClose : (c == '[' || c == ']') ? kStructBad : kStructNone;
    default: return d <= 1 ? kStructBad : kStructNone;
    }
}

// may token `nx` follow token `ty`?  [ [ {} , {} ] , [] ]: no comma missing, doubled or trailing, every bracket closed by its own
__device__ inline bool pair_allowed(int ty, int nx) {
    switch (ty) {
    case kTokAllOpen: return nx == kTokFamOpen || nx == kTokAllClose;
    case kTokFamOpen: return nx == kTokRecOpen || nx == kTokFamClose;
    case kTokRecOpen: return nx == kTokRecClose;
    case kTokRecClose: return nx == kTokCommaRec || nx == kTokFamClose;
    case kTokCommaRec: return nx == kTokRecOpen;
    case kTokFamClose: return nx == kTokCommaFam || nx == kTokAllClose;
    case kTokCommaFam: return nx == kTokFamOpen;
    default: return false;   // nothing follows the closing bracket of the families
    }
}

// ---- one record -----------------------------------------------------------------------------------------------------------
// The bytes of the file as a record walk sees them: from the LDS stage where the workgroup's range is staged ([lo, hi)),
// from global memory otherwise; behind `end` (the end of the families) there is nothing: a zero byte, which no rule accepts.
struct Src {
    const uint8_t *g, *st;
    uint32_t lo, hi, end;
    __device__ __forceinline__ uint32_t operator[](uint32_t i) const {
        if (i >= end) return 0;
        return (i - lo < hi - lo) ? st[i - lo] : g[i];
    }
};

// the sorted name table, and per entry the smallest 2 * record + side that uses it
struct NameTable {
    const uint8_t *bytes;
    const uint64_t *off;
    uint32_t n;
    uint32_t *first_use;
};

struct RecordOut {
    uint64_t *sds;        // [n][4] global left, global right, left_length, right_length
    uint64_t *chr_pos;    // [n][2]
    uint8_t *flags;       // [n] bit 0 reversed, bit 1 complemented, bit 2: the identity is hard (its span is the host's to convert)
    float *identity;      // [n]
    int32_t *chr;         // [n][2] index into the table; -1: a hard name (its span is the host's to decode)
    uint32_t *name_span;  // [n][2][2] start and length of the bytes between the quotes
    uint32_t *ident_span; // [n][2] start and length of the literal
};

struct RecordErr {
    uint32_t pos, rule;
};

constexpr int kFields = 13;
__device__ const char kFieldName[kFields][24] = {
    "chr_left", "chr_right", "global_left_position", "global_right_position", "chr_left_position", "chr_right_position",
    "left_length", "right_length", "left_seq", "right_seq", "identity", "reversed", "complemented"};
__device__ const uint8_t kFieldLen[kFields] = {8, 9, 20, 21, 17, 18, 11, 12, 8, 9, 8, 8, 12};
constexpr uint32_t kRequired = 0x1FFFu & ~(1u << 8) & ~(1u << 9);   // all but left_seq and right_seq
__device__ const double kPow10F64[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                         1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};   // each exact in f64

__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' < 10u; }
__device__ __forceinline__ uint32_t skip_ws(const Src &s, uint32_t i) {
    while (is_ws(s[i])) ++i;
    return i;
}
__device__ inline bool literal_at(const Src &s, uint32_t i, const char *text, uint32_t len) {
    for (uint32_t k = 0; k < len; ++k)
        if (s[i + k] != (uint8_t)text[k]) return false;
    return true;
}

// `0|[1-9][0-9]*` of at most 2^64 - 1 at i -> the value, i behind it
__device__ inline bool parse_u64(const Src &s, uint32_t &i, uint64_t &v) {
    uint32_t c = s[i];
    if (c == '0') {
        v = 0;
        ++i;
        return true;   // (a digit behind it is no comma: the caller refuses `01`)
    }
    if (!(c >= '1' && c <= '9')) return false;
    v = 0;
    while (is_digit(c = s[i])) {
        const uint64_t d = c - '0';
        if (v > (~0ull - d) / 10) return false;
        v = v * 10 + d;
        ++i;
    }
    return true;
}

// `-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?` at i -> i behind it.  The value is np.float32(float(literal)) where the
// conversion is exact: a significand of at most 2^53 and, the fraction digits folded in, a decimal exponent within +-22 make
// it ONE correctly rounded f64 multiply or divide by an exact power of ten, then the cast.  Everything else is hard.  A
// literal without fraction and exponent is an integer to the host's reader: `-0` is 0 and so +0.0, `-0.0` is -0.0.
__device__ inline bool parse_identity(const Src &s, uint32_t &i, float &value, bool &hard) {
    uint32_t p = i, c;
    const bool neg = s[p] == '-';
    if (neg) ++p;
    uint64_t sig = 0;
    uint32_t nd = 0, nfrac = 0;
    bool big = false, integer = true;
    auto push = [&](uint32_t ch) {
        if (sig == 0 && ch == '0') return;   // a leading zero
        if (nd < 19) sig = sig * 10 + (ch - '0'), ++nd;
        else big = true;
    };
    c = s[p];
    if (c == '0') {
        ++p;
    } else if (c >= '1' && c <= '9') {
        while (is_digit(c = s[p])) push(c), ++p;
    } else {
        return false;
    }
    // (digits of the integer part that were dropped as `big` would have to scale the exponent: such a literal is hard anyway)
    if (s[p] == '.') {
        integer = false;
        ++p;
        if (!is_digit(s[p])) return false;
        while (is_digit(c = s[p])) {
            push(c);
            if (nfrac < 100000) ++nfrac; else big = true;
            ++p;
        }
    }
    int32_t e = 0;
    if (s[p] == 'e' || s[p] == 'E') {
        integer = false;
        ++p;
        bool eneg = false;
        if (s[p] == '+' || s[p] == '-') eneg = s[p] == '-', ++p;
        if (!is_digit(s[p])) return false;
        while (is_digit(c = s[p])) {
            if (e < 100000) e = e * 10 + (int32_t)(c - '0'); else big = true;
            ++p;
        }
        if (eneg) e = -e;
    }
    i = p;
    const int32_t e10 = e - (int32_t)nfrac;
    hard = big || (sig != 0 && (sig > (1ull << 53) || e10 < -22 || e10 > 22));
    value = 0.0f;
    if (hard) return true;
    if (sig == 0) {
        value = (neg && !integer) ? -0.0f : 0.0f;
        return true;
    }
    double d = (double)sig;
    d = e10 < 0 ? d / kPow10F64[-e10] : d * kPow10F64[e10];
    value = (float)(neg ? -d : d);
    return true;
}

__device__ inline int cmp_name(const Src &s, uint32_t start, uint32_t len, const uint8_t *e, uint32_t elen) {
    const uint32_t m = min(len, elen);
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t a = s[start + k], b = e[k];
        if (a != b) return a < b ? -1 : 1;
    }
    return len < elen ? -1 : len > elen ? 1 : 0;
}

// the table entry whose bytes equal [start, start + len); -1: none
__device__ inline int32_t find_name(const Src &s, uint32_t start, uint32_t len, const NameTable &t) {
    uint32_t lo = 0, hi = t.n;   // first entry not below the name
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cmp_name(s, start, len, t.bytes + t.off[mid], (uint32_t)(t.off[mid + 1] - t.off[mid])) > 0) lo = mid + 1; else hi = mid;
    }
    if (lo < t.n && cmp_name(s, start, len, t.bytes + t.off[lo], (uint32_t)(t.off[lo + 1] - t.off[lo])) == 0) return (int32_t)lo;
    return -1;
}

// Record r, whose `{` is at `at`: every key and value once, in file order.  false: e names the first violation.
__device__ inline bool walk_record(const Src &s, uint32_t at, uint32_t r, const NameTable &table, const RecordOut &out,
                                   RecordErr &e, uint32_t &hard_names, uint32_t &hard_ident) {
    auto fail = [&](uint32_t pos, uint32_t rule) {
        e.pos = pos;
        e.rule = pos >= s.end ? (uint32_t)kRuleEnd : rule;
        return false;
    };
    uint32_t i = skip_ws(s, at + 1), seen = 0, flags = 0;
    if (s[i] == '}') return fail(i, kRuleMissing);
    for (;;) {
        if (s[i] != '"') return fail(i, kRuleKey);
        uint32_t len = 0;
        for (;; ++len) {
            const uint32_t c = s[i + 1 + len];
            if (c == '"') break;
            if (c == '\\' || c < 0x20 || len >= 22) return fail(i, kRuleKey);
        }
        int f = -1;
        for (int k = 0; k < kFields; ++k)
            if (len == kFieldLen[k] && literal_at(s, i + 1, kFieldName[k], len)) f = k;
        if (f < 0) return fail(i, kRuleKey);
        if (seen >> f & 1u) return fail(i, kRuleDup);
        seen |= 1u << f;
        i = skip_ws(s, i + len + 2);
        if (s[i] != ':') return fail(i, kRuleColon);
        i = skip_ws(s, i + 1);
        const uint32_t c = s[i];
        if (c == '{' || c == '[') return fail(i, kRuleNest);
        if (f <= 1) {   // chr_left, chr_right
            if (c != '"') return fail(i, kRuleName);
            uint32_t q = i + 1;
            bool escaped = false;
            for (;;) {
                const uint32_t ch = s[q];
                if (ch == '"') break;
                if (ch < 0x20) return fail(q, kRuleName);
                if (ch == '\\') escaped = true, ++q;   // (what it escapes is the host's to judge: the name is hard)
                ++q;
            }
            const uint32_t start = i + 1, n = q - start, slot = 2 * r + (uint32_t)f;
            const int32_t idx = escaped ? -1 : find_name(s, start, n, table);
            out.chr[slot] = idx;
            out.name_span[2 * slot] = start;
            out.name_span[2 * slot + 1] = n;
            if (idx >= 0) {
                if (table.first_use[idx] > slot) atomicMin(&table.first_use[idx], slot);   // (it only ever decreases)
            } else {
                ++hard_names;
            }
            i = q + 1;
        } else if (f <= 7) {   // the six positions and lengths
            uint64_t v;
            if (!parse_u64(s, i, v)) return fail(i, kRuleUint);
            uint64_t *dst = f == 2 ? out.sds + 4 * (size_t)r : f == 3 ? out.sds + 4 * (size_t)r + 1
                          : f == 4 ? out.chr_pos + 2 * (size_t)r : f == 5 ? out.chr_pos + 2 * (size_t)r + 1
                          : f == 6 ? out.sds + 4 * (size_t)r + 2 : out.sds + 4 * (size_t)r + 3;
            *dst = v;
        } else if (f <= 9) {   // left_seq, right_seq
            if (c == '"') return fail(i, kRuleSeq);
            if (!literal_at(s, i, "null", 4)) return fail(i, kRuleSeqNull);
            i += 4;
        } else if (f == 10) {
            float v;
            bool hard;
            const uint32_t start = i;
            if (!parse_identity(s, i, v, hard)) return fail(start, kRuleIdent);
            out.identity[r] = v;
            out.ident_span[2 * (size_t)r] = start;
            out.ident_span[2 * (size_t)r + 1] = i - start;
            if (hard) flags |= 4u, ++hard_ident;
        } else {   // reversed, complemented
            const uint32_t bit = f == 11 ? 1u : 2u;
            if (literal_at(s, i, "true", 4)) flags |= bit, i += 4;
            else if (literal_at(s, i, "false", 5)) i += 5;
            else return fail(i, kRuleBool);
        }
        i = skip_ws(s, i);
        if (s[i] == ',') {
            i = skip_ws(s, i + 1);
            continue;
        }
        if (s[i] == '}') break;
        return fail(i, f <= 7 && f >= 2 ? (uint32_t)kRuleUint : f == 10 ? (uint32_t)kRuleIdent : (uint32_t)kRuleComma);
    }
    if ((seen & kRequired) != kRequired) return fail(i, kRuleMissing);
    out.flags[r] = (uint8_t)flags;
    return true;
}

}  // namespace asgart
