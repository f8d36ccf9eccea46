// text_num_check.cpp -- csrc/text_num.h, the header text.hip compiles for the device, compiled for the host and held against
// glibc: the date of printdate() (gmtime_r + snprintf) and Netoutsv(), "%+5.1f" and "%03d" of (int)lvl.
// Usage: text_num_check <random cases>; prints "ok" or the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>

#include "text_num.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static bool check_date(long long sec, int usec)
{
    struct tm tmp;
    const time_t t = (time_t)sec;
    gmtime_r(&t, &tmp);
    char want[64], got[64];
    snprintf(want, sizeof(want), "%02d/%02d/%04d %02d:%02d:%02d.%03ld", tmp.tm_mday, tmp.tm_mon + 1, tmp.tm_year + 1900, tmp.tm_hour, tmp.tm_min,
             tmp.tm_sec, (long)usec / 1000);
    const TnDate d = tn_date(sec, usec);
    for (int j = 0; j < TN_DATE_LEN; ++j) got[j] = (char)tn_date_char(d, j);
    got[TN_DATE_LEN] = 0;
    if (strlen(want) != TN_DATE_LEN || strcmp(want, got) != 0) {
        printf("date %lld.%06d: want \"%s\" got \"%s\"\n", sec, usec, want, got);
        return false;
    }
    return true;
}

static bool check_level(float f)
{
    char want[80], got[80];
    snprintf(want, sizeof(want), "%+5.1f", f);
    const TnLevel l = tn_level(f);
    for (int j = 0; j < l.len && j < 79; ++j) got[j] = (char)tn_level_char(l, j);
    got[l.len < 79 ? l.len : 79] = 0;
    if (strcmp(want, got) != 0) {
        uint32_t u;
        memcpy(&u, &f, 4);
        printf("level %a (%08x): want \"%s\" got \"%s\"\n", f, u, want, got);
        return false;
    }
    // "%03d" of (int)f where the conversion is defined by the language; outside, the x86 result the header documents
    const bool in_int = f >= -2147483648.0f && f < 2147483648.0f;
    const int v = in_int ? (int)f : (-2147483647 - 1);
    snprintf(want, sizeof(want), "%03d", v);
    const JnTok t = tn_int0(tn_trunc_int(f), 3);
    for (int j = 0; j < t.len; ++j) got[j] = (char)jn_char(t, j);
    got[t.len] = 0;
    if (strcmp(want, got) != 0) {
        printf("(int)level %a: want \"%s\" got \"%s\"\n", f, want, got);
        return false;
    }
    return true;
}

static float bits_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 100000;
    // ---- dates: the named seconds, the days around every 28 February / 1 March of 2096 .. 2120, a dense sweep, random seconds
    const long long named[] = {1000000000ll, 2147483647ll, 2147483648ll, 4107542399ll, 4107542400ll, 4233686399ll, 4233686400ll, 4233772799ll, 4233772800ll,
                               4102444799ll, 4102444800ll, 0ll, 86399ll, 951782400ll, 4000000000ll + 703687441ll, 253402300799ll};
    for (long long s : named)
        for (int u : {0, 999, 1000, 499999, 999000, 999999})
            if (!check_date(s, u)) return 1;
    for (long long s = 1000000000ll - 86400; s < 4800000000ll; s += 86400 / 2 - 1)      // twice a day through 2122, the second drifting
        if (!check_date(s, (int)(s % 1000000))) return 1;
    for (long long s = 4107542400ll - 3 * 86400; s < 4107542400ll + 3 * 86400; s += 61)  // 2100-02-26 .. 03-03, every 61 s
        if (!check_date(s, 0)) return 1;
    for (long i = 0; i < n; ++i)
        if (!check_date((long long)(1000000000ull + rnd() % 3800000000ull), (int)(rnd() % 1000000ull))) return 1;
    // ---- levels: ties of the tenths, signed zeros, non-finite, the width's edges, random levels and random bit patterns
    const float named_f[] = {0.05f, -0.05f, 0.25f, -0.25f, 0.35f, -0.35f, -0.04f, 0.0f, -0.0f, 9.94f, 9.95f, 9.96f, -9.95f, -10.0f, 99.95f, -99.95f, -7.9f, 7.9f,
                             -0.9f, 0.99f, 999.95f, 3240.1f, -3240.1f, 2147483520.0f, 2147483648.0f, -2147483648.0f, -2147483904.0f, 8.9e17f, -8.9e17f,
                             INFINITY, -INFINITY, NAN, -NAN, bits_float(0x7fc00001u), bits_float(0xffc00001u), bits_float(1u), bits_float(0x80000001u)};
    for (float f : named_f)
        if (!check_level(f)) return 1;
    for (long i = -100000; i <= 100000; ++i)                                             // every tenth and every midpoint in +-5000
        if (!check_level((float)i / 20.0f)) return 1;
    for (long i = 0; i < n; ++i) {
        if (!check_level((float)((double)(rnd() % 66000000ull) / 10000.0 - 3300.0))) return 1;
        const float f = bits_float((uint32_t)rnd());
        if (std::isfinite(f) && std::fabs(f) >= 9e17f) continue;                          // (jn_level's domain)
        if (!check_level(f)) return 1;
    }
    printf("ok\n");
    return 0;
}
