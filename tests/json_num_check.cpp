// Host check of acarsdec_amd/csrc/json_num.h, the integer-arithmetic number printers the JSON kernels use, against glibc:
// cJSON's print_number recipe ("%1.15g", then "%1.17g" unless the text parses back) for the time stamp, snprintf(buf, 8,
// "%2.1f") for the level, "%d" for integers.  Built and run by tests/test_json_sink_model.py; prints the first mismatch.
#include <initializer_list>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "json_num.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void text(const JnTok& t, char* out)
{
    for (int j = 0; j < t.len; ++j) out[j] = (char)jn_char(t, j);
    out[t.len] = 0;
}

static int check_ts(long long sec, int usec)
{
    const double d = (double)sec + (double)usec / 1e6;
    char want[32], got[32];
    double back;
    snprintf(want, sizeof(want), "%1.15g", d);
    if (sscanf(want, "%lg", &back) != 1 || back != d) snprintf(want, sizeof(want), "%1.17g", d);
    text(jn_timestamp(sec, usec), got);
    if (strcmp(want, got)) {
        printf("timestamp %lld.%06d: glibc %s, json_num %s\n", sec, usec, want, got);
        return 1;
    }
    return 0;
}

static int check_level(float f)
{
    char want[8], got[32];
    snprintf(want, sizeof(want), "%2.1f", f);
    text(jn_level(f), got);
    if (strcmp(want, got)) {
        printf("level %a: glibc %s, json_num %s\n", f, want, got);
        return 1;
    }
    return 0;
}

int main(int argc, char** argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 200000;
    int bad = 0;
    const long long edge_sec[] = {1000000000ll, 1073741823ll, 1073741824ll, 2147483647ll, 2147483648ll, 2147483649ll, 4294967295ll,
                                  4294967296ll, 8589934592ll, 9999999997ll};
    for (long long s : edge_sec)
        for (int u = 0; u < 1000000 && bad < 5; u += 80) bad += check_ts(s, u);
    for (long long s : edge_sec)
        for (int u : {0, 1, 5, 499999, 500000, 500001, 999999}) bad += check_ts(s, u);
    for (long i = 0; i < n && bad < 5; ++i) {
        const long long sec = 1000000000ll + (long long)(rnd() % (i % 4 == 0 ? 8999999998ull : 3294967296ull));
        const int usec = i % 3 == 0 ? (int)(rnd() % 12500u) * 80 : (int)(rnd() % 1000000u);
        bad += check_ts(sec, usec);
    }
    // outside the exact domain: the integer second, bounded
    for (long long s : {-5ll, 0ll, 999999999ll, 9999999998ll, 123456789012345678ll}) {
        char got[32];
        text(jn_timestamp(s, 250000), got);
        if (strlen(got) > 15 || strspn(got, "0123456789") != strlen(got)) {
            printf("timestamp %lld outside the domain: %s\n", s, got);
            ++bad;
        }
    }
    const float ties[] = {0.05f, -0.05f, 0.25f, -0.25f, 0.35f, -0.35f, -0.04f, 0.f, -0.f, INFINITY, -INFINITY, NAN, -NAN, 9.95f, 99.95f,
                          -999.95f, 3240.1f, -3240.1f, 99999.9f, 123456.7f, -123456.7f, 1e9f, 1e-30f, -1e-45f};
    for (float f : ties) bad += check_level(f);
    for (long i = 0; i < n && bad < 5; ++i) {
        uint32_t u = (uint32_t)rnd();
        float f;
        if (i % 4 == 0) {                                   // any bit pattern below 9e17
            memcpy(&f, &u, 4);
            if (!(fabsf(f) < 9e17f)) continue;
        } else if (i % 4 == 1) {                            // tenths and their midpoints, where ties live
            f = (float)((double)((long)(rnd() % 200001u) - 100000) / 20.0);
        } else {
            f = (float)(((double)(rnd() % 2000000001ull) - 1e9) / 3e5);     // the range levels have
        }
        bad += check_level(f);
    }
    for (long long v : {0ll, 7ll, -1ll, 10ll, 99ll, 100ll, 1048575ll, 2147483647ll, -2147483648ll}) {
        char want[32], got[32];
        snprintf(want, sizeof(want), "%lld", v);
        text(jn_int(v), got);
        if (strcmp(want, got)) {
            printf("int %lld: %s\n", v, got);
            ++bad;
        }
    }
    if (!bad) printf("ok\n");
    return bad ? 1 : 0;
}
