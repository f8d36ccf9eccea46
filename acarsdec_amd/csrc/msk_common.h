// msk_common.h -- device helpers shared by the demodulator kernels (msk.hip: one wave per channel group; msk_lean.hip: the
// same with the framing taken off the per-bit path; msk2.hip: the stream split over two waves): constants of msk.c / acars.c,
// the channel state's way in and out of a launch, the LDS layout, the framing state machine (acars.c:239-375) and the one-bit
// step in front of it, the phase detector and loop filter, the mixer's sin/cos, the loop's f64 quotients and square root.
// Included by translation units built with -ffp-contract=off.
// The kernels sit next to a register cliff and are bound by the instructions they issue: a helper here is used by a kernel
// only where that kernel's instruction text is what it was with the piece spelled out (profiles/LEDGER.md).
#pragma once
#include <hip/hip_runtime.h>
#include "acg_internal.h"

#define FLEN 11
#define MFLTOVER 12

// acars.c:22-27
#define SYN 0x16
#define SOH 0x01
#define ETX 0x83
#define ETB 0x97
#define DLE 0x7f
#define MAXPERR 3

enum { WSYN = 0, SYN2, SOH1, TXT, CRC1, CRC2, END };   // acarsdec.h:88

#define K_TWOPI   (2.0 * 3.14159265358979323846)
#define K_3PI2    (3 * 3.14159265358979323846 / 2.0)
#define K_VCO     (1800.0 / 12500 * 2.0 * 3.14159265358979323846)      // msk.c:81

struct Lane {
    double phi, df, lvlsum;
    float clk;
    int bitcount;
    unsigned int S, idx;
    int nbits, astate, blen, berr;
    unsigned int outbits, crc0;
    long long nbit_total;
};

// the channel's record -> the state a launch carries (the ring and nsamp_total go their own way)
__device__ __forceinline__ void lane_load(Lane& L, const AcgChan* st)
{
    L.phi = st->phi; L.df = st->df; L.lvlsum = st->lvlsum;
    L.clk = st->clk; L.bitcount = st->bitcount; L.S = st->S; L.idx = st->idx;
    L.nbits = st->nbits; L.astate = st->astate; L.blen = st->blen; L.berr = st->berr;
    L.outbits = st->outbits; L.crc0 = st->crc0; L.nbit_total = st->nbit_total;
}

// inb[] -> the ring in LDS, every sample twice (rows k and k + FLEN: the matched filter's 11 taps never wrap); one lane per channel
template <int CPW>
__device__ __forceinline__ void ring_seed(float2 (*ring)[CPW], int slot, const AcgChan* st)
{
#pragma unroll
    for (int j = 0; j < FLEN; ++j) {
        const float2 x = make_float2(st->inb[2 * j], st->inb[2 * j + 1]);
        ring[j][slot] = x;
        ring[j + FLEN][slot] = x;
    }
}

// the state back into the channel's record after len samples more; p and idx are the loop's own copies of L.phi and L.idx; one
// lane per channel.  (The sum is formed here, behind the stores in front of it, where the kernels had it: formed at the call it
// is an instruction elsewhere in their write-back.)
__device__ __forceinline__ void lane_store(AcgChan* st, const Lane& L, double p, unsigned int idx, long long samp0, int len)
{
    st->phi = p; st->df = L.df; st->lvlsum = L.lvlsum;
    st->clk = L.clk; st->bitcount = L.bitcount; st->S = L.S; st->idx = idx;
    st->nbits = L.nbits; st->astate = L.astate; st->blen = L.blen; st->berr = L.berr;
    st->outbits = L.outbits; st->crc0 = L.crc0; st->nbit_total = L.nbit_total;
    st->nsamp_total = samp0 + len;
}

// the ring -> inb[]; one lane per channel
template <int CPW>
__device__ __forceinline__ void ring_save(AcgChan* st, const float2 (*ring)[CPW], int slot)
{
#pragma unroll
    for (int j = 0; j < FLEN; ++j) {
        const float2 x = ring[j][slot];
        st->inb[2 * j] = x.x;
        st->inb[2 * j + 1] = x.y;
    }
}

// the last workgroup out publishes the block-queue length of this launch to the host-mapped word of the call (no copy packet
// on the launch chain; the host reads it after the call's event).  WPG: waves per workgroup that have not met yet
template <int WPG>
__device__ __forceinline__ void publish_queue_length(const MskArgs& a)
{
    if (a.snap) {
        if (WPG > 1) __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            const unsigned int d = atomicAdd(a.done_ctr, 1u);
            if (d == gridDim.x - 1) {
                const unsigned int c = __hip_atomic_load(a.frame_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.snap, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(a.done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// LDS of the one-wave kernels.  inb[] of the wave's channels, every sample stored twice (k and k+FLEN) so that the 11 taps of
// the matched filter are always 11 consecutive rows starting at idx: no wrap, constant offsets.
// one struct = one layout: h[] first, so that its 11 reads h[o + 12 j] are immediate offsets (< 1 KiB) from the one
// address o * 4 (placed after the ring, every pair of reads needed its own base register)
template <int WPG, int CPW, int WSTR>
struct alignas(16) MskLds {
    float hs[(FLEN * MFLTOVER + 1 + 3) & ~3];
    double sc[2 * ACG_SINCOS_N];               // (cos, sin)(j * 2 pi / 128): the mixer's table, 2 KiB
    float2 ring_all[WPG][3 * FLEN + 1][CPW];   // rows 0..21: inb[] twice; rows 22 and 33: where lanes without a sample write
    float win_all[WPG][CPW][WSTR];             // sliding window of dm: blocks j and j+1
};

// h[] and the mixer's table into LDS, by a workgroup of NT threads
template <int NT>
__device__ __forceinline__ void lds_tables_load(float* hs, double* sc, const MskArgs& a)
{
    for (int i = threadIdx.x; i < FLEN * MFLTOVER + 1; i += NT) hs[i] = a.h[i];
    for (int i = threadIdx.x; i < 2 * ACG_SINCOS_N; i += NT) sc[i] = a.sctab[i];
}

__device__ __forceinline__ void reset_acars(Lane& L)          // acars.c:239-244
{
    L.astate = WSYN;
    L.df = 0;
    L.nbits = 1;
}

// soh_slot = &AcgChan::soh32 of the channel: the SOH stamp lives in the channel's state record in HBM, written and read by the
// group leader on these rare paths only.  (As a field of Lane it was one more value alive across the per-bit loop: the
// register allocator of this kernel's recipe started spilling -- ten scratch accesses in the loop, the demodulator alone 0.750
// -> 0.779 us per bit and 38 % slower beside the down-converter at 4096 channels; round 5, GPU calls 2-4.)
__device__ __forceinline__ void put_frame(Lane& L, const MskArgs& a, int ch, unsigned char crc1,
                                          const unsigned char* txt, long long sample_index, bool leader, unsigned int* soh_slot)
{
    // acars.c:350-369: queue the block.  lvl = 10*log10(MskLvlSum/MskBitCount) is taken on the host
    // from the two operands (same libm call as the reference).
    // the queue is a ring with a monotonic counter: the host consumes behind it (acg_collect_frames)
    if (leader) {
        const unsigned int slot = atomicAdd(a.frame_count, 1u);
        AcgFrameRec* f = a.frames + (slot & (a.frame_cap - 1));   // frame_cap is a power of two: consistent across the counter's wrap
        f->chn = ch;
        f->len = L.blen;
        f->err = L.berr;
        f->bitcount = L.bitcount;
        f->lvlsum = L.lvlsum;
        f->end_bit = L.nbit_total;
        f->end_sample = sample_index;
        f->crc[0] = (unsigned char)L.crc0;
        f->crc[1] = crc1;
        f->status = 0;
        f->pad[0] = 0;
        // where the reference stamps the block's time: at its SOH (acars.c:290 gettimeofday(&blk->tv)), as a distance back from
        // the closing bit (a block is < 2^16 samples long: the 32-bit difference is exact across the index's wrap)
        f->soh_back = (int)((unsigned int)sample_index - *soh_slot);
        const uint4* s = (const uint4*)txt;
        uint4* d = (uint4*)f->txt;
        const int nv = (L.blen + 15) >> 4;
        for (int i = 0; i < nv; ++i) d[i] = s[i];
    }
    L.astate = END;
    L.nbits = 8;
}

__device__ __forceinline__ void decode_acars(Lane& L, const MskArgs& a, int ch, unsigned char* txt,
                                             long long sample_index, bool leader, unsigned int* soh_slot)
{
    const unsigned int r = L.outbits & 0xffu;
    switch (L.astate) {
    case WSYN:                                                 // acars.c:252-265
        if (r == SYN) { L.astate = SYN2; L.nbits = 8; return; }
        if (r == (0xffu & ~SYN)) { L.S ^= 2; L.astate = SYN2; L.nbits = 8; return; }
        L.nbits = 1;
        return;
    case SYN2:                                                 // acars.c:267-279
        if (r == SYN) { L.astate = SOH1; L.nbits = 8; return; }
        if (r == (0xffu & ~SYN)) { L.S ^= 2; L.nbits = 8; return; }
        reset_acars(L);
        return;
    case SOH1:                                                 // acars.c:281-301
        if (r == SOH) {
            L.astate = TXT;
            L.blen = 0;
            L.berr = 0;
            L.nbits = 8;
            L.lvlsum = 0;
            L.bitcount = 0;
            if (leader) *soh_slot = (unsigned int)sample_index;    // acars.c:290: the block's time stamp is taken here
            return;
        }
        reset_acars(L);
        return;
    case TXT:                                                  // acars.c:303-341
        if (leader) txt[L.blen] = (unsigned char)r;
        L.blen++;
        if ((__popc(r) & 1) == 0) {
            L.berr++;
            if (L.berr > MAXPERR + 1) { reset_acars(L); return; }
        }
        if (r == ETX || r == ETB) { L.astate = CRC1; L.nbits = 8; return; }
        if (L.blen > 20 && r == DLE) {
            L.blen -= 3;
            L.crc0 = txt[L.blen];
            const unsigned char c1 = txt[L.blen + 1];
            L.astate = CRC2;
            put_frame(L, a, ch, c1, txt, sample_index, leader, soh_slot);
            return;
        }
        if (L.blen > 240) { reset_acars(L); return; }
        L.nbits = 8;
        return;
    case CRC1:                                                 // acars.c:343-347
        L.crc0 = r;
        L.astate = CRC2;
        L.nbits = 8;
        return;
    case CRC2:                                                 // acars.c:348-369
        put_frame(L, a, ch, (unsigned char)r, txt, sample_index, leader, soh_slot);
        return;
    default:                                                   // END, acars.c:370-373
        reset_acars(L);
        L.nbits = 8;
        return;
    }
}

// One decided bit through putbit (msk.c:53-63) and, when it closes a byte, decodeAcars (acars.c:246-375); sv is the soft bit
// under MskS & 2.  Two cases cover nearly every call and are taken without a branch: hunting for sync with no SYN in sight
// (acars.c:252-265, every bit of an idle channel) and a plain text byte -- good parity, no terminator, room left
// (acars.c:303-341, every 8th bit of a channel inside a block).  Everything else (sync, SOH, parity errors, ETX/ETB/DLE, CRC
// bytes, resets: a few per block) goes through the full state machine.
// CLOSES (msk_lean.hip, whose closing period is the one place it calls this): the closes behind a sync by selects as well -- on an
// idle channel a false sync comes about every 128 bits, and the byte behind it is the close that ends a segment there four times
// out of five, one lane taking its whole wave through the state machine's walk.  msk.hip and msk2.hip, which frame after EVERY bit,
// leave it off: the dozen selects per bit made msk.hip's kernel 5.4 % slower (profiles/LEDGER.md round 11).  ACG_LEAN_AB_CLOSE0
// is the text before, everywhere.
template <bool CLOSES = false>
__device__ __forceinline__ void frame_bit(Lane& L, float sv, const MskArgs& a, int ch, unsigned char* txt,
                                          long long sample_index, bool leader, unsigned int* soh_slot)
{
    {
        unsigned int ob = (L.outbits >> 1) & 0x7fu;
        if (sv > 0) ob |= 0x80u;
        L.outbits = ob;
    }
    L.nbits -= 1;
    {
        const bool ev = L.nbits <= 0;
        const unsigned int r = L.outbits & 0xffu;
        const bool syn = (r == SYN) | (r == (0xffu & ~SYN));
        const bool hunt = ev & (L.astate == WSYN) & !syn;
        const bool term = (r == ETX) | (r == ETB) | (r == DLE);
        const bool plain = ev & (L.astate == TXT) & ((__popc(r) & 1) != 0) & !term & (L.blen < 240);
        txt[plain ? L.blen : 255] = (unsigned char)r;          // byte 255 of the 256-byte text buffer is scratch (blen <= 241)
        L.blen += plain ? 1 : 0;
#ifdef ACG_LEAN_AB_CLOSE0
        constexpr bool closes = false;
#else
        constexpr bool closes = CLOSES;
#endif
        if constexpr (!closes) {
            L.nbits = hunt ? 1 : (plain ? 8 : L.nbits);
            if (ev & !hunt & !plain) decode_acars(L, a, ch, txt, sample_index, leader, soh_slot);
        } else {
            // The closes that end a segment of msk_lean.hip on idle channels, by selects as well: the byte behind a (mostly false) sync
            // -- SYN2 with SYN, ~SYN or neither (acars.c:267-279) --, a SOH1 that is no SOH (acars.c:299-300) and the byte behind a
            // block (acars.c:370-373).  Each sets the fields decode_acars() / reset_acars() set in that case.  What is left for the
            // state machine: a sync from WSYN, a SOH (time stamp), text bytes that are not plain, the CRC bytes.
            const unsigned int as = (unsigned int)L.astate;
            const bool s2 = ev & (as == SYN2);
            const bool s2miss = s2 & !syn;
            const bool s1miss = ev & (as == SOH1) & (r != SOH);
            const bool endc = ev & (as >= END);
            const bool rst = s2miss | s1miss | endc;               // reset_acars()
            const bool closed = s2 | s1miss | endc;
            if (ev & !hunt & !plain & !closed) {
                __builtin_assume(L.astate != SYN2 && (unsigned int)L.astate < END && (L.astate != SOH1 || r == SOH));
                decode_acars(L, a, ch, txt, sample_index, leader, soh_slot);
            }
            L.S ^= (s2 & (r == (0xffu & ~SYN))) ? 2u : 0u;
            L.astate = rst ? WSYN : ((s2 & (r == SYN)) ? SOH1 : L.astate);
            L.df = rst ? 0 : L.df;
            L.nbits = (hunt | s2miss | s1miss) ? 1 : ((plain | closed) ? 8 : L.nbits);
        }
    }
    L.nbit_total += 1;
    L.S += 1u;
}

// decision + phase detector, msk.c:115-121, as sign-bit arithmetic (exact: only signs move):
//   odd  S: vo = Im v, dphi = (vo >= 0) ? -Re v :  Re v
//   even S: vo = Re v, dphi = (vo >= 0) ?  Im v : -Im v
struct PhaseDet {
    float vo;           // soft bit before the MskS & 2 sign
    double dphi;
};

// (S, not its parity as a bool: handed over as a bool, the same operations come out of the compiler as other instructions)
__device__ __forceinline__ PhaseDet phase_detect(unsigned int S, float vr, float vi)
{
    const bool odd = (S & 1) != 0;
    PhaseDet d;
    d.vo = odd ? vi : vr;
    const float ot = odd ? vr : vi;
    const unsigned int flip = ((d.vo >= 0) == odd) ? 0x80000000u : 0u;
    d.dphi = (double)__uint_as_float(__float_as_uint(ot) ^ flip);
    return d;
}

// PLL filter, msk.c:130 (float constants promoted to double)
__device__ __forceinline__ double loop_filter(double df, double dphi)
{
    return (double)0.52f * df + (1.0 - (double)0.52f) * (double)38e-4f * dphi;
}

// sin/cos of x in [0, 2*pi) (any moderate |x| works): Cody-Waite reduction by pi/2 with a two-term
// constant, then the classic minimax kernels on |r| <= pi/4 (coefficients: fdlibm k_sin.c/k_cos.c,
// Sun Microsystems 1993, freely distributable; < 1 ulp).  The reference calls glibc's cexp (also
// < 1 ulp, different algorithm): results agree to the last bit except in rare last-place cases,
// and only the float-rounded product in*cos / in*sin is kept (msk.c:90).
// acc*z + C with the constant as an SGPR operand: one v_fma_f64.  (Left to the compiler, every Horner
// step becomes v_mov_b64 + v_fmac_f64 because the constant has to be copied into the accumulator.)
__device__ __forceinline__ double fma_zc(double acc, double z, double c)
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(acc), "v"(z), "s"(c));
    return r;
}

__device__ __forceinline__ void sincos_2pi(double x, double* sn, double* cs)
{
    const double kd = __builtin_rint(x * 6.36619772367581382433e-01);           // x * 2/pi
    const int q = (int)kd;
    double r = __builtin_fma(-kd, 1.57079632673412561417e+00, x);               // pi/2, high 33 bits
    r = __builtin_fma(-kd, 6.07710050650619224932e-11, r);                      // pi/2, tail
    const double z = r * r;
    // sin kernel
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    double ps = fma_zc(S6, z, S5);
    ps = fma_zc(ps, z, S4);
    ps = fma_zc(ps, z, S3);
    ps = fma_zc(ps, z, S2);
    const double v = z * r;
    const double s = __builtin_fma(v, fma_zc(ps, z, S1), r);
    // cos kernel
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double pc = fma_zc(C6, z, C5);
    pc = fma_zc(pc, z, C4);
    pc = fma_zc(pc, z, C3);
    pc = fma_zc(pc, z, C2);
    pc = fma_zc(pc, z, C1);
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    const double c = w + (((1.0 - w) - hz) + z * (z * pc));
    // quadrant
    const double ss = (q & 1) ? c : s;
    const double cc = (q & 1) ? s : c;
    *sn = (q & 2) ? -ss : ss;
    *cs = ((q + 1) & 2) ? -cc : cc;
}

// The mixer's sin/cos as the product ships it: a 128-entry table of (cos, sin)(j * 2 pi / 128) in LDS (correctly rounded
// doubles, acg_host_sincos_table) and a rotation by the small remainder |r| <= pi / 128,
//     cos p = cj + (cj (cos r - 1) - sj sin r),    sin p = sj + (sj (cos r - 1) + cj sin r),
// with sin r - r and cos r - 1 from three-term series (next terms < 4e-19 relative).  23 vector instructions and one LDS
// read instead of ~40 for sincos_2pi above (no quadrant logic, shorter polynomials) on a loop that is bound by the number
// of instructions it issues.  Error <= 2.1 ulp (the table entry's and the last addition's rounding dominate)
// where sincos_2pi has < 1; what the demodulator keeps is (float)(in * cos), (float)(in * -sin) (msk.c:90), and on 4e7 random
// phases those are identical to glibc cexp's for both (tests/sincos_model.c: the same operations on the CPU, in the CPU suite).
// (in two parts, so that a caller can issue the table read early and run the series behind other work: msk_lean.hip)
__device__ __forceinline__ void sincos_tab_entry(double x, const double* __restrict__ tab, double* rr, double* cj, double* sj);
__device__ __forceinline__ void sincos_tab_rotate(double r, double cj, double sj, double* sn, double* cs);

__device__ __forceinline__ void sincos_tab(double x, const double* __restrict__ tab /* LDS, [128][2] */, double* sn, double* cs)
{
    double r, cj, sj;
    sincos_tab_entry(x, tab, &r, &cj, &sj);
    sincos_tab_rotate(r, cj, sj, sn, cs);
}

__device__ __forceinline__ void sincos_tab_entry(double x, const double* __restrict__ tab /* LDS, [128][2] */, double* rr, double* cj, double* sj)
{
    const double kd = __builtin_rint(x * (6.36619772367581382433e-01 * 32.0));   // x * 128 / (2 pi)
    const int q = (int)kd;
    double r = __builtin_fma(-kd, 1.57079632673412561417e+00 / 32.0, x);        // 2 pi / 128, high 33 bits (exact products: kd <= 128)
    r = __builtin_fma(-kd, 6.07710050650619224932e-11 / 32.0, r);               // tail
    const double2 e = *(const double2*)(tab + 2 * (q & (ACG_SINCOS_N - 1)));
    *rr = r;
    *cj = e.x;
    *sj = e.y;
}

__device__ __forceinline__ void sincos_tab_rotate(double r, double cj, double sj, double* sn, double* cs)
{
    const double z = r * r;
    double ps = __builtin_fma(z, -1.98412698412698412698e-04, 8.33333333333333333333e-03);
    ps = __builtin_fma(z, ps, -1.66666666666666666667e-01);
    const double sm = (r * z) * ps;                                              // sin r - r
    double pc = __builtin_fma(z, -1.38888888888888888889e-03, 4.16666666666666666667e-02);
    pc = __builtin_fma(z, pc, -0.5);
    const double cm1 = z * pc;                                                   // cos r - 1
    const double sr = r + sm;
    const double u = __builtin_fma(cj, cm1, -(sj * sr));
    const double w = __builtin_fma(sj, cm1, cj * sr);
    *cs = cj + u;
    *sn = sj + w;
}

// z * c + d as ONE three-address v_fma_f64, c a scalar operand and d a register that is left alone (left to the compiler the step
// is v_mov_b64 + v_fmac_f64: d copied into the accumulator)
__device__ __forceinline__ double fma_zsv(double z, double c, double d)
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(z), "s"(c), "v"(d));
    return r;
}

// sincos_tab_rotate with the three Horner steps whose constant addend the compiler copies into the accumulator as three-address
// fmas (fma_zsv twice, fma_zc once): the same operations on the same operands, three register copies fewer (msk_lean.hip; msk.hip
// and msk2.hip keep the text they have)
__device__ __forceinline__ void sincos_tab_rotate3(double r, double cj, double sj, double* sn, double* cs)
{
    const double z = r * r;
    double ps = fma_zsv(z, -1.98412698412698412698e-04, 8.33333333333333333333e-03);
    ps = fma_zc(ps, z, -1.66666666666666666667e-01);
    const double sm = (r * z) * ps;                                              // sin r - r
    double pc = fma_zsv(z, -1.38888888888888888889e-03, 4.16666666666666666667e-02);
    pc = __builtin_fma(z, pc, -0.5);
    const double cm1 = z * pc;                                                   // cos r - 1
    const double sr = r + sm;
    const double u = __builtin_fma(cj, cm1, -(sj * sr));
    const double w = __builtin_fma(sj, cm1, cj * sr);
    *cs = cj + u;
    *sn = sj + w;
}

// n0 / d and n1 / d, both correctly rounded, for d in [1e-8, ~1e2] and |n| < ~1e2 or n == +0 (the matched filter's
// sum starts from +0 and so is never -0, the one numerator whose quotient would come out as +0 here): see the call site.
// acg_selftest_div2 compares it with the compiler's IEEE division on the device.
__device__ __forceinline__ void div2_shared_rcp(double n0, double n1, double d, double* q0, double* q1)
{
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
    const double a = n0 * r, b = n1 * r;
    *q0 = __builtin_fma(__builtin_fma(-d, a, n0), r, a);
    *q1 = __builtin_fma(__builtin_fma(-d, b, n1), r, b);
}

// one quotient, same construction (the tap phase clk / s, msk.c:103: s ~ 0.9, |clk| < 1)
__device__ __forceinline__ double div1_rcp(double n, double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
    const double a = n * r;
    return __builtin_fma(__builtin_fma(-d, a, n), r, a);
}

// sqrt(x), correctly rounded, for x = 0 or x in [1e-100, 1e100]: the compiler's own expansion (rsq, one coupled
// Newton step on (g, h) = (sqrt, 1 / (2 sqrt)), two remainder steps) without the exponent scaling it wraps around
// it for arguments below 2^-767.  |v|^2 (msk.c:110 through cabsf) is a sum of two squares of floats.
__device__ __forceinline__ double sqrt_rn_positive(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
    g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
    return g;
}

__device__ __forceinline__ double sqrt_rn_midrange(double x)
{
    return x == 0.0 ? x : sqrt_rn_positive(x);
}

// (float)sqrt(x) for x = a*a + b*b of two floats: such an x is 0 or >= 2^-298, and everything below 2^-300 has the float
// square root 0 -- so the zero case is one v_max_f64 (sqrt(1e-300) = 1e-150 -> 0.0f) instead of compare + two selects,
// or worse a branch around the Newton steps: any branch inside the bit decision splits its basic block, and each split
// measured ~3 % per bit (the scheduler fills latency slots only within a block)
__device__ __forceinline__ float sqrtf_of_sum_of_squares(double x)
{
    return (float)sqrt_rn_positive(__builtin_fmax(x, 1e-300));
}

// msk.c:83 `if (p >= 2*M_PI) p -= 2*M_PI;` as compare + one select + one fma: fma(-1, 2pi, p) is p - 2pi
// with its single rounding, fma(-0.0, 2pi, p) is p itself (p + -0.0), and -1.0 / -0.0 differ in the high
// word only.  Same results, one instruction less than subtract + two-word select on the serial chain
// (measured: the three-level form "difference beside compare, then a two-word select" is 4 % slower per bit --
// the loop is bound by the number of instructions it issues, not by the depth of this chain).
__device__ __forceinline__ double wrap_2pi(double p)
{
    const double k = __hiloint2double(p >= K_TWOPI ? (int)0xBFF00000 : (int)0x80000000, 0);
    return __builtin_fma(k, K_TWOPI, p);
}

