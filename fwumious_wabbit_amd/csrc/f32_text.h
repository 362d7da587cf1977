// Decimal text -> f32 for the device text route (textparse.hip), compiled for the host as well (fwgpu_f32_from_text).
//
// The grammar is parse_f32_rust's (parser.cpp), which is Rust's f32::from_str: [+-]? (digits [. digits?] | . digits)
// [(e|E) [+-]? digits], or inf / infinity / nan in any case.  The function returns whether the text is in the grammar,
// the f32 bits, and `proven`: set only when the bits are those of the correctly rounded value (strtof).  A caller that
// needs the reference's result and sees proven == 0 asks the host.
//
// How a result is proven.  Up to 19 significant digits go into a u64 m, the rest are dropped (relative error < 2^-59).
// With the decimal exponent e, |e| <= 44, a double d ~ m * 10^e comes from at most one int -> double conversion and two
// operations with exact powers of ten (10^k is exact for k <= 22), each correctly rounded: d is within 4 double ulps of
// the value.  (float)d differs from the correctly rounded value only if a midpoint of two neighbouring floats lies
// between d and the value, that is within 4 double ulps of d; midpoints of normal floats (and FLT_MAX + half an ulp) are
// the doubles whose low 29 mantissa bits are 0x10000000.  So: proven unless those bits are within kWindow of that
// pattern.  When m < 2^53 and |e| <= 22, d is the correctly rounded double (Clinger's fast path) and only d ON the midpoint
// is in doubt -- and not even then when d is exact (e == 0, m * 10^e below 2^53, or 5^-e divides m), where round-half-even is right.
// Results below the smallest normal float, at or above 2^128, special spellings and longer exponents stay unproven.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FWGPU_HD __host__ __device__
#else
#define FWGPU_HD
#endif

namespace fwgpu {

struct F32Text {
    uint32_t bits;
    bool grammar;  // the text is an f32 in the grammar above
    bool proven;   // bits == strtof(text)
};

FWGPU_HD static inline double f32_text_pow10(int k) {  // exact for 0 <= k <= 22
    const double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                          1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return t[k];
}

FWGPU_HD static inline bool f32_text_word(const unsigned char *s, size_t n, const char *w, size_t l) {
    if (n != l) return false;
    for (size_t j = 0; j < l; j++) {
        unsigned char c = s[j];
        if (c >= 'A' && c <= 'Z') c = (unsigned char)(c - 'A' + 'a');
        if (c != (unsigned char)w[j]) return false;
    }
    return true;
}

FWGPU_HD static inline F32Text f32_from_text(const unsigned char *s, size_t n) {
    F32Text r{0u, false, false};
    if (n == 0 || n > 4096) return r;
    size_t i = 0;
    bool neg = false;
    if (s[0] == '+' || s[0] == '-') {
        neg = s[0] == '-';
        i = 1;
    }
    if (i == n) return r;
    if (f32_text_word(s + i, n - i, "inf", 3) || f32_text_word(s + i, n - i, "infinity", 8)) {
        r.grammar = true;
        r.bits = neg ? 0xff800000u : 0x7f800000u;
        return r;
    }
    if (f32_text_word(s + i, n - i, "nan", 3)) {
        r.grammar = true;
        r.bits = 0x7fc00000u;
        return r;
    }
    uint64_t m = 0;
    int nsig = 0, nd = 0;
    int e10 = 0;  // decimal exponent that goes with m
    while (i < n && s[i] >= '0' && s[i] <= '9') {
        const unsigned d = s[i] - '0';
        if (nsig < 19) {
            if (m || d) m = m * 10 + d, nsig++;
        } else if (e10 < 100000) {
            e10++;  // a dropped integer digit
        }
        i++, nd++;
    }
    if (i < n && s[i] == '.') {
        i++;
        while (i < n && s[i] >= '0' && s[i] <= '9') {
            const unsigned d = s[i] - '0';
            if (nsig < 19) {
                if (m || d) m = m * 10 + d, nsig++;
                if (e10 > -100000) e10--;
            }
            i++, nd++;
        }
    }
    if (nd == 0) return r;
    if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        bool eneg = false;
        if (i < n && (s[i] == '+' || s[i] == '-')) {
            eneg = s[i] == '-';
            i++;
        }
        int ex = 0, ne = 0;
        while (i < n && s[i] >= '0' && s[i] <= '9') {
            if (ex < 100000) ex = ex * 10 + (s[i] - '0');
            i++, ne++;
        }
        if (ne == 0) return r;
        e10 += eneg ? -ex : ex;
    }
    if (i != n) return r;
    r.grammar = true;
    const uint32_t sign = neg ? 0x80000000u : 0u;
    if (m == 0) {
        r.bits = sign;
        r.proven = true;
        return r;
    }
    if (e10 < -44 || e10 > 44) return r;
    const bool fast = m < (1ull << 53) && e10 >= -22 && e10 <= 22;
    double d = (double)m;
    bool exact = false;
    if (e10 == 0) {
        exact = fast;
    } else if (e10 > 0) {
        d *= f32_text_pow10(e10 > 22 ? 22 : e10);
        if (e10 > 22) d *= f32_text_pow10(e10 - 22);
        exact = fast && d < 9007199254740992.0;  // an integer product below 2^53 was not rounded
    } else {
        const int k = -e10;
        d /= f32_text_pow10(k > 22 ? 22 : k);
        if (k > 22) d /= f32_text_pow10(k - 22);
    }
    uint64_t db;
    memcpy(&db, &d, 8);
    const int be = (int)((db >> 52) & 0x7ff) - 1023;
    const float f = (float)d;
    uint32_t fb;
    memcpy(&fb, &f, 4);
    r.bits = fb | sign;
    if (be < -126 || be > 127) return r;  // subnormal or zero float, or at / beyond 2^128
    const int64_t low = (int64_t)(db & 0x1fffffffull) - 0x10000000ll;
    const int64_t dist = low < 0 ? -low : low;
    const int64_t kWindow = 8;
    if (fast && dist == 0 && e10 < 0) {  // m / 10^k on a midpoint: exact when 5^k divides m (the division by 2^k always is)
        uint64_t p5 = 1;
        for (int k = 0; k < -e10; k++) p5 *= 5;  // 5^22 < 2^52
        exact = m % p5 == 0;
    }
    r.proven = fast ? (dist != 0 || exact) : dist > kWindow;
    return r;
}

}  // namespace fwgpu
