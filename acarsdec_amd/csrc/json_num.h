// json_num.h -- the numbers of a JSON line (json.hip) as integer arithmetic: what cJSON's print_number (cJSON.c:475-506) prints
// for buildjson()'s time stamp, and what "%2.1f" prints for the level (output.c:244-251).  Host and device compile the same
// functions, so that a host program can hold them against glibc's printf / strtod (tests/json_num_check.cpp).
//
// A token is [-] integer digits [. fraction digits]; jn_char() gives its j-th character, so that the lanes of a wave write a
// token without anybody walking a digit string.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define JN_FN __host__ __device__ __forceinline__
#else
#define JN_FN static inline
#endif

struct JnTok {
    uint64_t ip, fr;            // integer part; fraction as an integer of fr_digits digits
    int neg, ip_digits, fr_digits, fr_shown;   // fr_shown <= fr_digits leading fraction digits are printed (0: no point either)
    int special;                // 0, or 1 = "inf", 2 = "nan" (after the sign)
    int len;
};

JN_FN uint64_t jn_pow10(int e)
{
    uint64_t p = 1;
    for (int i = 0; i < e; ++i) p *= 10u;
    return p;
}

JN_FN int jn_digits(uint64_t v)
{
    int n = 1;
    while (v >= 10u) { v /= 10u; ++n; }
    return n;
}

JN_FN unsigned char jn_char(const JnTok& t, int j)
{
    if (j < t.neg) return '-';
    j -= t.neg;
    if (t.special == 1) return (unsigned char)(j == 0 ? 'i' : j == 1 ? 'n' : 'f');
    if (t.special == 2) return (unsigned char)(j == 1 ? 'a' : 'n');
    if (j < t.ip_digits) return (unsigned char)('0' + (t.ip / jn_pow10(t.ip_digits - 1 - j)) % 10u);
    if (j == t.ip_digits) return '.';
    return (unsigned char)('0' + (t.fr / jn_pow10(t.fr_digits - 1 - (j - t.ip_digits - 1))) % 10u);
}

// "%d"
JN_FN JnTok jn_int(long long v)
{
    JnTok t;
    t.neg = v < 0;
    t.ip = t.neg ? 0ull - (uint64_t)v : (uint64_t)v;
    t.fr = 0;
    t.ip_digits = jn_digits(t.ip);
    t.fr_digits = t.fr_shown = t.special = 0;
    t.len = t.neg + t.ip_digits;
    return t;
}

// x * 10^p / 2^s rounded half-even on the exact value (x * 10^p < 2^63)
JN_FN uint64_t jn_round_shift(uint64_t x, int s)
{
    uint64_t q = x >> s;
    const uint64_t r = x & ((1ull << s) - 1ull), half = 1ull << (s - 1);
    if (r > half || (r == half && (q & 1ull))) ++q;
    return q;
}

// print_number (cJSON.c:475-506) of t = (double)sec + (double)usec / 1e6: "%1.15g", and "%1.17g" when that text does not parse
// back to t.  For 10^9 <= t < 10^10 - 1 the double is I + k / 2^s with ten integer digits and s = 23 .. 19, so %1.15g shows 5
// and %1.17g 7 fraction digits: N = k 10^p / 2^s rounded half-even on the exact value (glibc rounds the exact binary value),
// trailing zeros stripped (%g), and the 15-digit text parses back to t iff it lies within half an ulp of t,
//     2 |N 2^s - k 10^5| < 10^5,   or equal with k even (strtod's ties go to the even neighbour).
// (k = 0 prints the integer, which parses back exactly: the narrower half-interval below a power of two never matters.)
// Everything stays below 2^48.  Outside that domain (a clock before 2001 or after 2286) the token is the integer second,
// clamped to 0 .. 10^15 - 1: well formed and bounded, not the reference's digits.
JN_FN JnTok jn_timestamp(long long sec, int usec)
{
    JnTok t;
    t.neg = t.special = 0;
    t.fr = 0;
    t.fr_digits = t.fr_shown = 0;
    const double d = (double)sec + (double)usec / 1e6;
    if (!(sec >= 1000000000ll && sec < 9999999998ll && usec >= 0 && usec < 1000000)) {
        t.ip = sec < 0 ? 0ull : sec > 999999999999999ll ? 999999999999999ull : (uint64_t)sec;
        t.ip_digits = jn_digits(t.ip);
        t.len = t.ip_digits;
        return t;
    }
    uint64_t bits;
    memcpy(&bits, &d, 8);
    const int s = 52 - ((int)((bits >> 52) & 0x7ffu) - 1023);         // 23 .. 19
    const uint64_t mant = (bits & ((1ull << 52) - 1ull)) | (1ull << 52);
    uint64_t I = mant >> s;
    const uint64_t k = mant & ((1ull << s) - 1ull);
    int p = 5;
    uint64_t N = jn_round_shift(k * 100000ull, s);
    const uint64_t a = N << s, b = k * 100000ull, dist = a > b ? a - b : b - a;
    if (!(2ull * dist < 100000ull || (2ull * dist == 100000ull && !(k & 1ull)))) {
        p = 7;
        N = jn_round_shift(k * 10000000ull, s);
    }
    if (N == jn_pow10(p)) {                                            // the fraction rounded up to the next second
        ++I;
        N = 0;
    }
    int shown = p;
    for (uint64_t v = N; shown > 0 && v % 10u == 0; v /= 10u) --shown;  // %g strips trailing zeros (and then the point)
    t.ip = I;
    t.ip_digits = jn_digits(I);
    t.fr = N;
    t.fr_digits = p;
    t.fr_shown = shown;
    t.len = t.ip_digits + (shown ? 1 + shown : 0);
    return t;
}

// snprintf(convert_tmp, 8, "%2.1f", f) (output.c:250): (double)f * 10 is exact (24 + 4 bits), rint of it is round-half-even on
// the exact value as glibc's, the sign is the sign bit ("-0.0" for -0.04), and the 8-byte buffer cuts the text to 7 characters.
// Exact for |f| < 9e17; a level is 10 log10 of a double, |f| < 3241 or not finite ("inf", "-inf", "nan", "-nan" as glibc).
JN_FN JnTok jn_level(float f)
{
    JnTok t;
    uint32_t u;
    memcpy(&u, &f, 4);
    t.neg = (int)(u >> 31);
    t.ip = t.fr = 0;
    t.ip_digits = t.fr_digits = t.fr_shown = t.special = 0;
    if (((u >> 23) & 0xffu) == 0xffu) {
        t.special = (u & 0x7fffffu) ? 2 : 1;
        t.len = t.neg + 3;
        return t;
    }
    u &= 0x7fffffffu;
    float af;
    memcpy(&af, &u, 4);
    double a = (double)af * 10.0;
    if (a > 9e18) a = 9e18;
    const uint64_t N = (uint64_t)__builtin_rint(a);
    t.ip = N / 10u;
    t.ip_digits = jn_digits(t.ip);
    t.fr = N % 10u;
    t.fr_digits = t.fr_shown = 1;
    t.len = t.neg + t.ip_digits + 2;
    if (t.len > 7) t.len = 7;
    return t;
}
