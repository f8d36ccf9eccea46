// text_num.h -- the numbers of a text record (text.hip) as integer arithmetic, beside json_num.h: printdate()'s
// "%02d/%02d/%04d %02d:%02d:%02d.%03ld" of gmtime_r (output.c:138-160; Netoutsv's date is its first 19 characters,
// netout.c:128-133), "%+5.1f" of the level (output.c:168-172,338), "%03d" of (int)lvl (netout.c:134) and "%0Nd" in general.
// Host and device compile the same functions, so that a host program can hold them against glibc (tests/text_num_check.cpp).
// As in json_num.h a token's j-th character is computed, so that the lanes of a wave write it without walking a digit string.
#pragma once
#include "json_num.h"

// gmtime_r's calendar fields of a time_t as one decimal number DDMMYYYYhhmmss (14 digits) from integer civil-from-days
// arithmetic: days since 1970-01-01 -> (year, month, day) of the proleptic Gregorian calendar, which knows that 2100 is no leap
// year (t0 < 4 * 10^9 s plus 2^43 samples of 80 us reaches 2118).  Exact for 0 <= sec < 253402300800 (the year 10000: "%04d"
// holds); outside, sec is clamped into that range (well formed, not the reference's digits).
// printdate() prints nothing when tv_sec + tv_usec == 0; with sec >= 10^9 (acg_text_enable's range for t0) that cannot happen.
struct TnDate {
    uint64_t dmyhms;            // DDMMYYYYhhmmss
    int ms;                     // tv_usec / 1000
};

JN_FN TnDate tn_date(long long sec, int usec)
{
    if (sec < 0) sec = 0;
    if (sec > 253402300799ll) sec = 253402300799ll;
    const uint64_t days = (uint64_t)sec / 86400u, sod = (uint64_t)sec % 86400u;
    // civil_from_days (days >= 0): eras of 400 years = 146097 days, counted from 0000-03-01
    const uint64_t z = days + 719468u;
    const uint64_t era = z / 146097u, doe = z % 146097u;                          // [0, 146096]
    const uint64_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;   // [0, 399]
    const uint64_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);              // [0, 365], the year starts in March
    const uint64_t mp = (5u * doy + 2u) / 153u;                                   // [0, 11]
    const uint64_t d = doy - (153u * mp + 2u) / 5u + 1u;
    const uint64_t m = mp < 10u ? mp + 3u : mp - 9u;
    const uint64_t y = yoe + era * 400u + (m <= 2u ? 1u : 0u);
    TnDate t;
    t.dmyhms = ((((d * 100u + m) * 10000u + y) * 100u + sod / 3600u) * 100u + (sod / 60u) % 60u) * 100u + sod % 60u;
    t.ms = usec < 0 ? 0 : usec > 999999 ? 999 : usec / 1000;
    return t;
}

#define TN_DATE_LEN 23          // "DD/MM/YYYY hh:mm:ss.mmm"
#define TN_DATE_SV_LEN 19       // "DD/MM/YYYY hh:mm:ss"

// character j (0 .. 22) of "%02d/%02d/%04d %02d:%02d:%02d.%03ld"
JN_FN unsigned char tn_date_char(const TnDate& t, int j)
{
    if (j == 2 || j == 5) return '/';
    if (j == 10) return ' ';
    if (j == 13 || j == 16) return ':';
    if (j == 19) return '.';
    if (j > 19) return (unsigned char)('0' + ((uint64_t)t.ms / jn_pow10(22 - j)) % 10u);
    const int d = j - (j > 2) - (j > 5) - (j > 10) - (j > 13) - (j > 16);         // digit 0 .. 13 of DDMMYYYYhhmmss
    return (unsigned char)('0' + (t.dmyhms / jn_pow10(13 - d)) % 10u);
}

// "%0Nd": jn_int with the digit count raised to the width (the leading digits of a shorter number are zeros)
JN_FN JnTok tn_int0(long long v, int width)
{
    JnTok t = jn_int(v);
    if (t.neg + t.ip_digits < width) t.ip_digits = width - t.neg;
    t.len = t.neg + t.ip_digits;
    return t;
}

// (int)lvl as the reference's x86 build converts it (cvttss2si): toward zero, and the "integer indefinite" -2147483648 for a NaN,
// an infinity and everything outside int
JN_FN int tn_trunc_int(float f)
{
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (-2147483647 - 1);
}

// "%+5.1f" of a float: jn_level's digits (the exact value rounded half-even to one decimal, no 7-character cut), a forced sign,
// padded with spaces to 5.  Non-finite as glibc: "+inf", "-inf", "+nan", "-nan", padded alike.  Exact for |f| < 9e17 as jn_level;
// a level is 10 log10 of a double, |f| < 3241 or not finite.  pad = the spaces in front; len = pad + sign + digits.
struct TnLevel {
    JnTok t;                    // the digits, t.neg = 0: the sign is written apart
    int neg, pad, len;
};

JN_FN TnLevel tn_level(float f)
{
    TnLevel l;
    l.t = jn_level(f);
    l.neg = l.t.neg;
    l.t.neg = 0;
    l.t.len = l.t.special ? 3 : l.t.ip_digits + 2;
    l.pad = l.t.len + 1 < 5 ? 5 - (l.t.len + 1) : 0;
    l.len = l.pad + 1 + l.t.len;
    return l;
}

JN_FN unsigned char tn_level_char(const TnLevel& l, int j)
{
    if (j < l.pad) return ' ';
    if (j == l.pad) return (unsigned char)(l.neg ? '-' : '+');
    return jn_char(l.t, j - l.pad - 1);
}
