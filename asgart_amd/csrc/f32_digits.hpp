// f32_digits.hpp -- the shortest decimal digits of an f32 and the two forms the result files print them in.
//
// f32_shortest_digits follows the published description of Schubfach (R. Giulietti, "The Schubfach way to render
// doubles", 2020), specialised to f32 and written for this library.  For v = c * 2^q (c < 2^24) let R be the set of reals
// that round to v: from (c - 1/2) 2^q to (c + 1/2) 2^q, the lower end at (c - 1/4) 2^q where v is a power of two above the
// smallest normal (its lower neighbour is half as far), both ends included iff c is even (a reader rounds ties to even).
// With k = floor(log10 of R's width), 10^k <= width < 10^(k+1): R holds at least one multiple of 10^k and at most one of
// 10^(k+1).  That one, when it exists, is the answer (every shorter candidate is a multiple of 10^(k+1) too); otherwise
// the answer is the multiple of 10^k in R closest to v, which is s or s + 1 for s = floor(v / 10^k), ties to even s.
//
// Every comparison is made on integers: the three values 4 c' 2^q 10^-k for c' the lower end, v and the upper end (in
// units of 2^(q-2)) are computed ROUNDED TO ODD -- floor(x) with the lowest bit set when x is no integer -- which keeps
// every comparison with an even integer, and those are all there are.  10^-k comes from a table of 128-bit significands
// (pow10_table, computed with integer arithmetic when the library is first used):
//   k <= 0   10^|k| = 5^|k| 2^|k| exactly (5^45 < 2^105), so the product is exact and any fraction bit is the sticky bit;
//   k > 0    ceil(2^e / 5^k): the product is too large by less than c' 2^-sh <= 2^-98 (sh >= 124 below), while a true
//            product c' 2^(q-k) / 5^k (q > k here) is an integer or at least 5^-31 > 2^-72 away from one: fraction bits
//            below 2^-90 are rounding noise and are ignored, the bits above decide.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace asgart {

constexpr int kPow10Min = -45, kPow10Max = 31;  // the k of 10^-k an f32 can ask for: floor(-149 log10 2) .. floor(104 log10 2)
constexpr int kPow10Entries = kPow10Max - kPow10Min + 1;
constexpr int kF32TextMax = 64;                 // bytes a rendered f32 can take (the longest, -0.0000...0117549435, is 49)

struct Pow10Entry {   // 10^-k = (hi:lo) * 2^x: exactly when exact != 0, otherwise rounded up; 2^127 <= hi:lo < 2^128
    uint64_t hi, lo;
    int64_t x;
    uint64_t exact;
};

// ---- the table (host, integer arithmetic only) ---------------------------------------------------------------------------
inline void build_pow10_table(Pow10Entry *t) {
    typedef unsigned __int128 u128;
    auto bit_length = [](u128 v) {
        int b = 0;
        while (v) {
            ++b;
            v >>= 1;
        }
        return b;
    };
    for (int k = kPow10Min; k <= kPow10Max; ++k) {
        Pow10Entry &e = t[k - kPow10Min];
        u128 p5 = 1;
        for (int i = 0; i < (k < 0 ? -k : k); ++i) p5 *= 5;
        u128 g;
        if (k <= 0) {   // 10^|k| = (5^|k| << z) * 2^(|k| - z)
            const int z = 128 - bit_length(p5);
            g = p5 << z;
            e.x = -k - z;
            e.exact = 1;
        } else {        // 10^-k ~ ceil(2^e2 / 5^k) * 2^(-e2 - k), e2 = 127 + bits of 5^k: the quotient has 128 bits
            const int e2 = 127 + bit_length(p5);
            u128 quo = 0, rem = 0;
            for (int i = e2; i >= 0; --i) {   // long division of 2^e2, one bit at a time (rem < 5^k < 2^72)
                rem = (rem << 1) | (i == e2 ? 1u : 0u);
                quo <<= 1;
                if (rem >= p5) {
                    rem -= p5;
                    quo |= 1;
                }
            }
            g = quo + (rem != 0 ? 1 : 0);
            e.x = -e2 - k;
            e.exact = 0;
        }
        e.hi = (uint64_t)(g >> 64);
        e.lo = (uint64_t)g;
    }
}

inline const Pow10Entry *pow10_table() {
    static const struct Table {
        Pow10Entry e[kPow10Entries];
        Table() { build_pow10_table(e); }
    } table;
    return table.e;
}

// ---- digits ------------------------------------------------------------------------------------------------------------------
enum : uint32_t { kF32Finite = 0, kF32Zero = 1, kF32Inf = 2, kF32NaN = 3 };

struct F32Digits {
    uint32_t digits;  // the decimal digits as a number, no trailing zero; < 10^9
    uint32_t nd;      // how many there are (1..9)
    int32_t kk;       // the value is 0.DIGITS * 10^kk
    uint32_t cls;     // kF32Finite (digits, nd, kk are valid), kF32Zero, kF32Inf, kF32NaN
    uint32_t neg;     // the sign bit
};

__host__ __device__ inline void mul_64x64(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// cp * g / 2^sh rounded to odd; cp < 2^26, 124 <= sh <= 128, the result is below 2^30
__host__ __device__ inline uint32_t scaled_round_to_odd(const Pow10Entry &g, uint32_t cp, int sh) {
    uint64_t a_hi, a_lo, b_hi, b_lo;
    mul_64x64(cp, g.lo, a_hi, a_lo);
    mul_64x64(cp, g.hi, b_hi, b_lo);
    const uint64_t w0 = a_lo, w1 = a_hi + b_lo, w2 = b_hi + (w1 < a_hi ? 1 : 0);   // the product, 64 bits a word
    const int s0 = sh - 64;                                                        // 60 .. 64
    const uint64_t whole = s0 >= 64 ? w2 : (w2 << (64 - s0)) | (w1 >> s0);
    const uint64_t frac1 = s0 >= 64 ? w1 : w1 & (((uint64_t)1 << s0) - 1);
    const bool sticky = frac1 != 0 || (g.exact ? w0 != 0 : (w0 >> (sh - 90)) != 0);
    return (uint32_t)whole | (sticky ? 1u : 0u);
}

__host__ __device__ inline uint32_t decimal_length_u32(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}

__host__ __device__ inline F32Digits f32_shortest_digits(float v, const Pow10Entry *__restrict__ table) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, v);
    const uint32_t t = bits & 0x7FFFFFu, bq = (bits >> 23) & 0xFFu;
    F32Digits out{0, 0, 0, kF32Finite, bits >> 31};
    if (bq == 0xFFu) {
        out.cls = t ? kF32NaN : kF32Inf;
        return out;
    }
    if (bq == 0 && t == 0) {
        out.cls = kF32Zero;
        return out;
    }
    const int q = bq ? (int)bq - 150 : -149;
    const uint32_t c = bq ? (t | 0x800000u) : t;
    const bool narrow = t == 0 && bq > 1;   // a power of two whose lower neighbour is half as far
    // floor(q log10 2) and floor(q log10 2 + log10(3/4)), exact for |q| <= 150: 1262611 / 2^22 = 0.3010299206 (log10 2 =
    // 0.3010299957, off by 1.2e-5 at most over the range; no q log10 2 [- 0.1249] comes that close to an integer)
    const int k = narrow ? (q * 1262611 - 524031) >> 22 : (q * 1262611) >> 22;
    const Pow10Entry g = table[k - kPow10Min];
    const int sh = -(q + (int)g.x);
    const uint32_t par = c & 1u, cb = c << 2;
    const uint32_t vb = scaled_round_to_odd(g, cb, sh);
    const uint32_t vbl = scaled_round_to_odd(g, narrow ? cb - 1 : cb - 2, sh);
    const uint32_t vbr = scaled_round_to_odd(g, cb + 2, sh);
    const uint32_t s = vb >> 2;
    const uint32_t sp = s / 10 * 10, tp = sp + 10;            // the multiples of 10^(k+1) around v
    const bool sp_in = vbl + par <= (sp << 2), tp_in = (tp << 2) + par <= vbr;
    uint32_t d;
    if (sp_in != tp_in) {
        d = sp_in ? sp : tp;
    } else {
        const uint32_t s1 = s + 1;
        const bool s_in = vbl + par <= (s << 2), s1_in = (s1 << 2) + par <= vbr;
        if (s_in != s1_in) {
            d = s_in ? s : s1;
        } else {   // both in R: the closer one, a tie to the even one
            const int32_t cmp = (int32_t)vb - (int32_t)((s + s1) << 1);
            d = (cmp < 0 || (cmp == 0 && (s & 1u) == 0)) ? s : s1;
        }
    }
    int e = k;
    while (d % 10 == 0) {   // (d > 0: the lower end of R is above 0)
        d /= 10;
        ++e;
    }
    out.digits = d;
    out.nd = decimal_length_u32(d);
    out.kk = (int32_t)out.nd + e;
    return out;
}

// ---- the two forms -------------------------------------------------------------------------------------------------------------
// A sink takes bytes one after the other: byte(c), lit("..."), zeros(n).  render_f32 writes
//   serde_json's form (json = true; ryu's pretty printer behind serde_json::to_string_pretty, src/exporters.rs:12-25, what
//   postprocess.f32_repr states): `null` for NaN and the infinities, `0.0` / `-0.0`, positional with at least `.0` for
//   1e-5 <= |v| < 1e13 (decimal point position -6 < kk <= 13), otherwise d[.ddd]e[-]x;
//   Rust's `{}` (json = false; `write!(.., "{}", sd.identity)`, src/exporters.rs:44 and :92, what slice.f32_display states):
//   `NaN`, `inf`, `-inf`, `0`, `-0`, always positional, a fraction only where there is one.
template <class Sink>
__host__ __device__ inline void render_digits(Sink &s, uint32_t digits, uint32_t nd, uint32_t from, uint32_t to) {
    // digits [from, to) of the nd digits, left to right
    uint32_t v = digits;
    for (uint32_t i = to; i < nd; ++i) v /= 10;   // drops the digits behind `to`
    uint64_t nib = 0;                             // one nibble per digit: digit `from` ends up lowest
    for (uint32_t i = from; i < to; ++i) {
        nib = nib << 4 | v % 10;
        v /= 10;
    }
    for (uint32_t i = from; i < to; ++i) {
        s.byte((uint8_t)('0' + (uint32_t)(nib & 15u)));
        nib >>= 4;
    }
}

template <class Sink>
__host__ __device__ inline void render_f32(Sink &s, const F32Digits &d, bool json) {
    if (d.cls == kF32NaN) {
        if (json) s.lit("null"); else s.lit("NaN");
        return;
    }
    if (d.cls == kF32Inf) {
        if (json) {
            s.lit("null");
        } else {
            if (d.neg) s.byte('-');
            s.lit("inf");
        }
        return;
    }
    if (d.neg) s.byte('-');
    if (d.cls == kF32Zero) {
        if (json) s.lit("0.0"); else s.byte('0');
        return;
    }
    const int kk = d.kk, nd = (int)d.nd;
    if (json && !(-6 < kk && kk <= 13)) {   // d[.ddd]e[-]x, x = kk - 1
        render_digits(s, d.digits, d.nd, 0, 1);
        if (nd > 1) {
            s.byte('.');
            render_digits(s, d.digits, d.nd, 1, d.nd);
        }
        s.byte('e');
        int x = kk - 1;
        if (x < 0) {
            s.byte('-');
            x = -x;
        }
        if (x >= 10) s.byte((uint8_t)('0' + x / 10));
        s.byte((uint8_t)('0' + x % 10));
        return;
    }
    if (kk >= nd) {            // an integer: the digits, then zeros
        render_digits(s, d.digits, d.nd, 0, d.nd);
        s.zeros((uint32_t)(kk - nd));
        if (json) s.lit(".0");
    } else if (kk > 0) {       // the point inside the digits
        render_digits(s, d.digits, d.nd, 0, (uint32_t)kk);
        s.byte('.');
        render_digits(s, d.digits, d.nd, (uint32_t)kk, d.nd);
    } else {                   // 0.000ddd
        s.lit("0.");
        s.zeros((uint32_t)(-kk));
        render_digits(s, d.digits, d.nd, 0, d.nd);
    }
}

}  // namespace asgart
