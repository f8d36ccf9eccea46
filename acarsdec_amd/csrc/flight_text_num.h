// flight_text_num.h -- the numbers of the monitor screen (flight_text.hip) as integer arithmetic, beside json_num.h and
// text_num.h: printtime()'s "%02d:%02d:%02d.%03ld" of gmtime_r(tv_sec) and tv_usec / 1000 (output.c:138-146) and printmonitor()'s
// "%3d" of the message count (output.c:471).  The route line's "timestamp" is json_num.h's jn_timestamp as it stands.
// Host and device compile the same functions, so that a host program can hold them against glibc (tests/flight_text_num_check.cpp).
// As there, a token's j-th character is computed: the lanes of a wave write it without walking a digit string.
#pragma once
#include "text_num.h"

#define FTN_TIME_LEN 12         // "hh:mm:ss.mmm"

// printtime() is the tail of printdate()'s text: characters 11 .. 22 of "DD/MM/YYYY hh:mm:ss.mmm" (text_num.h), with its range
// (exact for 0 <= sec < the year 10000, 2100 no leap year; outside, sec is clamped) and its tv_usec / 1000
JN_FN unsigned char ftn_time_char(const TnDate& t, int j)
{
    return tn_date_char(t, TN_DATE_LEN - FTN_TIME_LEN + j);
}

// "%3d": jn_int's digits behind max(0, 3 - their count) spaces; never cut (1000 takes four places, -2147483648 eleven)
struct FtnInt3 {
    JnTok t;
    int pad, len;
};

JN_FN FtnInt3 ftn_int3(int v)
{
    FtnInt3 n;
    n.t = jn_int(v);
    n.pad = n.t.len < 3 ? 3 - n.t.len : 0;
    n.len = n.pad + n.t.len;
    return n;
}

JN_FN unsigned char ftn_int3_char(const FtnInt3& n, int j)
{
    return j < n.pad ? (unsigned char)' ' : jn_char(n.t, j - n.pad);
}
