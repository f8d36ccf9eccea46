// sink_put.h -- the row writers of the device renderers (json.hip, text.hip, flight_text.hip), one copy.  A wave assembles one record
// in an LDS row and lane j writes character j; one function both measures and renders, so every writer is templated on
//   W   write; otherwise only measure (the same positions are computed, nothing is stored);
//   B   the row's bound: no store lands at or behind row[B].
// Each returns the position behind what it put.  Every function is inlined into the kernels of the unit that includes it.  A unit
// may bind its own bound in one line (#define PUT_LIT(s) PK_PUT_LIT(B, s)); what only one format uses ("%Ns" padding, the date,
// the unescaped text) stays in that format's unit and stores through pk_st.
#pragma once
#include "sink_pack.h"
#include "json_num.h"

// characters [from, from + 16) of a literal
constexpr PkLit pk_lit_part(const char* s, unsigned int from)
{
    unsigned int n = 0;
    while (s[n]) ++n;
    char part[17] = {};
    for (unsigned int i = 0; i < 16 && from + i < n; ++i) part[i] = s[from + i];
    return pk_lit(part);
}

template <bool W, unsigned int B>
__device__ __forceinline__ void pk_st(unsigned char* row, unsigned int p, unsigned char v)
{
    if (W && p < B) row[p] = v;                                    // (the bound holds by construction; this keeps a bug inside the row)
}

template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int pk_put_lit(unsigned char* row, unsigned int pos, const PkLit l, int lane)
{
    if (W && (unsigned int)lane < l.n) pk_st<W, B>(row, pos + lane, (unsigned char)((lane < 8 ? l.lo : l.hi) >> (8 * (lane & 7))));
    return pos + l.n;
}
// a literal of at most 64 characters at `pos` of `row` (W, pos, row and lane are the calling function's)
#define PK_PUT_LIT(B, s) do { static_assert(sizeof(s) - 1 <= 64, "literal"); \
                              constexpr PkLit a_ = pk_lit_part(s, 0); pos = pk_put_lit<W, B>(row, pos, a_, lane); \
                              if (sizeof(s) - 1 > 16) { constexpr PkLit b_ = pk_lit_part(s, 16); pos = pk_put_lit<W, B>(row, pos, b_, lane); } \
                              if (sizeof(s) - 1 > 32) { constexpr PkLit c_ = pk_lit_part(s, 32); pos = pk_put_lit<W, B>(row, pos, c_, lane); } \
                              if (sizeof(s) - 1 > 48) { constexpr PkLit d_ = pk_lit_part(s, 48); pos = pk_put_lit<W, B>(row, pos, d_, lane); } } while (0)

// n <= 64 copies of c
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int pk_fill(unsigned char* row, unsigned int pos, unsigned char c, unsigned int n, int lane)
{
    if (W && (unsigned int)lane < n) pk_st<W, B>(row, pos + lane, c);
    return pos + n;
}

template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int pk_put_tok(unsigned char* row, unsigned int pos, const JnTok& t, int lane)
{
    if (W && lane < t.len) pk_st<W, B>(row, pos + lane, jn_char(t, lane));
    return pos + (unsigned int)t.len;
}

// the C string at s (at most maxlen < 64 bytes): the lane's byte in *b (0 at or behind its end), its length returned
__device__ __forceinline__ int pk_strlen(const unsigned char* s, int maxlen, int lane, unsigned int* b)
{
    *b = lane < maxlen ? s[lane] : 0u;
    const unsigned long long nul = __ballot(*b == 0);             // (never 0: maxlen < 64)
    return __ffsll((unsigned long long)nul) - 1;
}

// n bytes that are already escaped (the station and app stretches), 4-byte aligned: a dword load per lane, not a load per byte
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int pk_put_words(unsigned char* row, unsigned int pos, const unsigned char* src, unsigned int n, int lane)
{
    if (W)
        for (unsigned int i = 4u * lane; i < n; i += 256) {
            const unsigned int w = *(const unsigned int*)(src + i);
#pragma unroll
            for (unsigned int k = 0; k < 4; ++k)
                if (i + k < n) pk_st<W, B>(row, pos + i + k, (unsigned char)(w >> (8 * k)));
        }
    return pos + n;
}

// ---- cJSON's string escape: print_string_ptr's classes (cJSON.c:858-877).  A byte's place is its index + the two-character escapes
// before it + 5 x the \u00xx escapes before it: two ballots and two popcounts, never a lane walking the string.
__device__ __forceinline__ bool pk_two(unsigned int b)
{
    return b == '"' || b == '\\' || b == '\b' || b == '\f' || b == '\n' || b == '\r' || b == '\t';
}

// one lane's byte, escaped, at p
template <bool W, unsigned int B>
__device__ __forceinline__ void pk_put_escaped(unsigned char* row, unsigned int p, unsigned int b, bool two, bool six)
{
    if (!W) return;
    if (two) {
        pk_st<W, B>(row, p, '\\');
        pk_st<W, B>(row, p + 1, (unsigned char)(b == '\b' ? 'b' : b == '\f' ? 'f' : b == '\n' ? 'n' : b == '\r' ? 'r' : b == '\t' ? 't' : b));
    } else if (six) {                                              // sprintf("u%04x"): lower-case hex, b < 32
        pk_st<W, B>(row, p, '\\');
        pk_st<W, B>(row, p + 1, 'u');
        pk_st<W, B>(row, p + 2, '0');
        pk_st<W, B>(row, p + 3, '0');
        pk_st<W, B>(row, p + 4, (unsigned char)('0' + (b >> 4)));
        const unsigned int lo = b & 15u;
        pk_st<W, B>(row, p + 5, (unsigned char)(lo < 10 ? '0' + lo : 'a' + lo - 10));
    } else {
        pk_st<W, B>(row, p, (unsigned char)b);
    }
}

// up to 64 bytes of a string whose lane's byte is b (0 = at or behind its end): `live` lanes are those before the first NUL.
// Returns the escaped length; *more = no NUL among the 64 (the string goes on in the next round).
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int pk_put_round(unsigned char* row, unsigned int pos, unsigned int b, int lane, bool* more)
{
    const unsigned long long nul = __ballot(b == 0);
    const int n = nul ? __ffsll((unsigned long long)nul) - 1 : 64;
    const bool live = lane < n;
    const bool two = live && pk_two(b), six = live && b < 32u && !two;
    const unsigned long long m2 = __ballot(two), m6 = __ballot(six), below = (1ull << lane) - 1ull;
    if (live) pk_put_escaped<W, B>(row, pos + (unsigned int)lane + (unsigned int)__popcll(m2 & below) + 5u * (unsigned int)__popcll(m6 & below), b, two, six);
    *more = n == 64;
    return (unsigned int)n + (unsigned int)__popcll(m2) + 5u * (unsigned int)__popcll(m6);
}

// "<C string at s, at most maxlen < 64 bytes>" escaped as print_string_ptr does
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int pk_put_str(unsigned char* row, unsigned int pos, const unsigned char* s, int maxlen, int lane)
{
    const unsigned int b = lane < maxlen ? s[lane] : 0u;
    bool more;
    if (lane == 0) pk_st<W, B>(row, pos, '"');
    const unsigned int n = pk_put_round<W, B>(row, pos + 1, b, lane, &more);
    if (lane == 0) pk_st<W, B>(row, pos + 1 + n, '"');
    return pos + n + 2;
}
