// flight_text_num_check.cpp -- csrc/flight_text_num.h, the header flight_text.hip compiles for the device, compiled for the host
// and held against glibc: printtime()'s token (gmtime_r + snprintf "%02d:%02d:%02d.%03ld") and printmonitor()'s "%3d".
// Usage: flight_text_num_check <random cases>; prints "ok" or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <initializer_list>

#include "flight_text_num.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static bool check_time(long long sec, int usec)
{
    struct tm tmp;
    const time_t t = (time_t)sec;
    gmtime_r(&t, &tmp);
    char want[64], got[64];
    snprintf(want, sizeof(want), "%02d:%02d:%02d.%03ld", tmp.tm_hour, tmp.tm_min, tmp.tm_sec, (long)usec / 1000);
    const TnDate d = tn_date(sec, usec);
    for (int j = 0; j < FTN_TIME_LEN; ++j) got[j] = (char)ftn_time_char(d, j);
    got[FTN_TIME_LEN] = 0;
    if (strlen(want) != FTN_TIME_LEN || strcmp(want, got) != 0) {
        printf("time %lld.%06d: want \"%s\" got \"%s\"\n", sec, usec, want, got);
        return false;
    }
    return true;
}

static bool check_int3(int v)
{
    char want[32], got[32];
    snprintf(want, sizeof(want), "%3d", v);
    const FtnInt3 n = ftn_int3(v);
    for (int j = 0; j < n.len && j < 31; ++j) got[j] = (char)ftn_int3_char(n, j);
    got[n.len < 31 ? n.len : 31] = 0;
    if (strcmp(want, got) != 0) {
        printf("%%3d of %d: want \"%s\" got \"%s\"\n", v, want, got);
        return false;
    }
    return true;
}

int main(int argc, char** argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 100000;
    // ---- the time token: a day's last and first second, tv_sec at and past 2^31 and 2^32, the usec edges; sweeps; random
    const long long named[] = {1700006399ll, 1700006400ll, 1000000000ll, 2147483647ll, 2147483648ll, 4294967295ll, 4294967296ll, 4294967301ll, 8589934592ll,
                               4107542399ll, 4107542400ll, 0ll, 86399ll, 86400ll, 253402300799ll};
    for (long long s : named)
        for (int u : {0, 999, 1000, 499999, 999000, 999999})
            if (!check_time(s, u)) return 1;
    for (long long s = 1700006400ll - 7200; s < 1700006400ll + 7200; ++s)                 // every second around a midnight
        if (!check_time(s, (int)(s % 1000000))) return 1;
    for (long long s = 1000000000ll; s < 9000000000ll; s += 86400 / 2 - 1)                 // twice a day, the second drifting, past 2^33
        if (!check_time(s, (int)(s % 1000000))) return 1;
    for (long i = 0; i < n; ++i)
        if (!check_time((long long)(1000000000ull + rnd() % 8000000000ull), (int)(rnd() % 1000000ull))) return 1;
    // ---- "%3d"
    const int ints[] = {1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 2147483647, 0, -1, -9, -10, -99, -100, -2147483647 - 1};
    for (int v : ints)
        if (!check_int3(v)) return 1;
    for (int v = -2000; v <= 20000; ++v)
        if (!check_int3(v)) return 1;
    for (long i = 0; i < n; ++i)
        if (!check_int3((int)(uint32_t)rnd())) return 1;
    printf("ok\n");
    return 0;
}
