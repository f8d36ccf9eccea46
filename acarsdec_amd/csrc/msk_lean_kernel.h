// msk_lean_kernel.h -- the text of msk_lean_kernel<LPC, WPG, LOG>, for the two units that instantiate it: msk_lean.hip (4 and 8 lanes
// per channel, both workgroup shapes; its head comment describes the kernel) and msk_lean_wide.hip (16 lanes per channel).
// To be included behind msk_common.h.
#pragma once

// P = 2 P + (bit of `mask` for this lane): one v_addc_co_u32 (the lane mask of a compare is the carry-in)
__device__ __forceinline__ unsigned int shift_in(unsigned int P, bool b)
{
    const unsigned long long m = __builtin_amdgcn_ballot_w64(b);
    unsigned int r;
    unsigned long long co;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(co) : "v"(P), "s"(m));
    return r;
}

template <int LPC, int WPG, bool LOG>
__global__ __launch_bounds__(64 * WPG) void msk_lean_kernel(const MskArgs a)
{
    constexpr int CPW = 64 / LPC;                  // channels per wave
    constexpr int SPL = (6 + LPC - 1) / LPC;       // mixer samples per lane per bit period
    constexpr int WB = 64;                         // dm samples per refill block (msk.hip)
    constexpr int SPB = WB / LPC;
    constexpr int WSTR = 2 * WB + 4;
    constexpr int SEG = 8;                         // bit periods per segment: 6 SEG <= WB - 1, and <= 8 so that a segment closes at most one byte
    constexpr int NREC = (SEG + LPC - 1) / LPC;    // bit records of a segment a lane keeps (records g, g + LPC, ...)
    static_assert(6 * (SEG + 1) <= WB - 1 && 12 * (SEG + 1) <= 2 * WB - 1, "a segment and its closing period stay inside the dm window");
    static_assert(LPC == 4 || LPC == 8 || LPC == 16, "lane groups of 4, 8 or 16 (a lane moves whole float4s of the dm window: SPB >= 4)");
    static_assert(SEG >= 1 && SEG <= 8, "a segment closes at most one byte");
    __shared__ MskLds<WPG, CPW, WSTR> lds;
    float* hs = lds.hs;
    lds_tables_load<64 * WPG>(hs, lds.sc, a);

    const int wv = threadIdx.x >> 6;
    const int tid = threadIdx.x & 63;
    float2 (*ring)[CPW] = lds.ring_all[wv];
    float (*win)[WSTR] = lds.win_all[wv];
    const int slot = tid / LPC;
    const int g = tid - slot * LPC;
    const int ch0 = (blockIdx.x * WPG + wv) * CPW; // first channel of this wave
    const int ch = ch0 + slot;
    const bool active = ch < a.nch;
    const bool leader = (g == 0) && active;
    // slots beyond the last channel (last wave only) REPLICATE the last channel: same input, same state, side effects by the
    // real group's leader only -- so that every lane of a wave with work fires its bits (the segment test below is wave-wide)
    const int chc = active ? ch : a.nch - 1;
    AcgChan* st = a.st + chc;

    Lane L;
    lane_load(L, st);
    L.outbits &= 0xffu;
    const long long samp0 = st->nsamp_total;
    const long long nbt_in = L.nbit_total;
    if (g == 0) ring_seed<CPW>(ring, slot, st);

    const float* __restrict__ dm = a.dm + (size_t)chc * a.dm_pitch;
    unsigned char* txt = a.txt + (size_t)chc * 256;
    const int len = ch0 < a.nch ? a.len : 0;       // (a wave without any channel -- padding of a 4-wave workgroup -- idles)
    // LOG (ACG_F_BITLOG): the per-bit records {soft symbol, level} of msk.hip, every lane of a group storing the identical record
    float2* const bits = LOG ? a.bits + (size_t)chc * a.bit_cap : nullptr;
    int nb = (LOG && a.bit_append) ? a.nbits_out[chc] : 0;
    int n = 0;
    unsigned int idx = L.idx;
    double p = L.phi;

    // ---- dm window (msk.hip): lane g owns samples [g*SPB, (g+1)*SPB) of every block of WB
    float pend[SPB];
    const int limv = a.len >= SPB ? a.len - SPB : 0;
    typedef float f4v __attribute__((ext_vector_type(4)));
    auto fetch_block = [&](int blk) {
        const int base = blk * WB + g * SPB;
        const f4v* src = (const f4v*)(dm + (base < limv ? base : limv));
#pragma unroll
        for (int q = 0; q < SPB; q += 4) {
            const f4v v = src[q / 4];
            pend[q] = v.x; pend[q + 1] = v.y; pend[q + 2] = v.z; pend[q + 3] = v.w;
        }
    };
    f4v* const wrow = (f4v*)&win[slot][g * SPB];
    auto store_block = [&](int blk) {
        f4v* w = wrow + (blk & 1) * (WB / 4);
#pragma unroll
        for (int q = 0; q < SPB; q += 4) w[q / 4] = f4v{pend[q], pend[q + 1], pend[q + 2], pend[q + 3]};
    };
    fetch_block(0);
    store_block(0);
    fetch_block(1);
    store_block(1);
    fetch_block(2);
    int pend_blk = 2;
    int refill_at = WB;
    __syncthreads();

    if (a.high_prio) __builtin_amdgcn_s_setprio(3);
    // every kernel argument the epilogue needs is loaded HERE: a scalar load still pending when the loop starts makes the compiler
    // wait with a zero count inside the segment's first period (scalar loads return out of order), behind that period's h[] reads
    asm volatile("" :: "s"(a.snap), "s"(a.done_ctr));

    typedef float f2v __attribute__((ext_vector_type(2)));
// holds a VCO / clock step where the source has it: an empty statement that the compiler must take to read and write the step's
// phase and clock and the lane's pick (nothing is issued for it), so that neither sinking nor the scheduler carries the step past
// it.  Steps 5 and 6 always carry one; steps 1-4 only where steps 5 and 6 are under the branch (ACG_LEAN_AB_SPEC0)
#ifdef ACG_LEAN_AB_PICK0
#define LEAN_HOLD_STEP(pv, cv, mv) asm volatile("" : "+v"(pv), "+v"(cv))
#else
#define LEAN_HOLD_STEP(pv, cv, mv) asm volatile("" : "+v"(pv), "+v"(cv), "+v"(mv))
#endif
// the hold of step 5 leaves the clock out (round 10): the sixth step's hold keeps both clock steps in the block anyway, and with the
// fifth clock step free to move, its operations fill the two slots that the phase chain's tail in front of the hold cost as
// `s_nop 0` (a compare's lane mask is read two instructions later at the earliest, a wrap fma's sum one later)
#if defined(ACG_LEAN_AB_NOP0) || defined(ACG_LEAN_AB_PICK0)
#define LEAN_HOLD_STEP5(pv, cv, mv) LEAN_HOLD_STEP(pv, cv, mv)
#else
#define LEAN_HOLD_STEP5(pv, cv, mv) asm volatile("" : "+v"(pv), "+v"(mv))
#endif
#define MSK_TAP(j, x) (f2v{(j & 1) ? hv2[j / 2].y : hv2[j / 2].x, (j & 1) ? hv2[j / 2].y : hv2[j / 2].x} * x)
// `s_waitcnt lgkmcnt(n)` alone (gfx9 encoding: the other counters at their maximum)
#define LEAN_WAIT_LGKM(n) __builtin_amdgcn_s_waitcnt(0xC07F | ((n) << 8))

    // what a period's front part (VCO / clock steps, mixer, the five oldest filter taps) hands to its bit decision
    int cnt;
    bool fired;
    float clk_f;
    f2v hv2[(FLEN + 1) / 2];
    f2v acc;
    float2 xs[FLEN - 5];                           // the six newest taps' ring entries, read by front() right behind its ring write

    // ---- front part of a bit period: msk.hip phases A, C0, B, operation for operation
    auto front = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float in_cur[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) in_cur[j] = win[slot][(n + g + j * LPC) & (2 * WB - 1)];

        const double s = K_VCO + L.df;                                     // msk.c:81
        const double thr = K_3PI2 - s / 2;                                 // msk.c:96
        double myp[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) myp[j] = p;
        cnt = 0;
        fired = false;
        double p4 = p;
        float c4 = L.clk;
        double pq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            p4 += s;
            p4 = wrap_2pi(p4);
            c4 = (float)((double)c4 + s);
            pq[u] = p4;
#if defined(ACG_LEAN_AB_SPEC0) && !defined(ACG_LEAN_AB_VCO0)
            // (only where steps 5 and 6 are under the branch: there machine sinking moves the phase step after them otherwise)
            LEAN_HOLD_STEP(p4, c4, myp[(u > 0 ? u - 1 : 0) / LPC]);
#endif
#ifndef ACG_LEAN_AB_PICK0
            // (a lane that is not `quick` or has no sample left mixes these into the ring's spare row, except its first sample,
            // whose phase is this one: the one-sample branch below computes the same p + s)
            if ((u % LPC) == g) myp[u / LPC] = p4;
#endif
        }
        const bool quick = (s > 0) && !((double)c4 >= thr) && (n + 6 <= len);
#ifndef ACG_LEAN_AB_SPEC0
        // steps 5 and 6 of both chains in the same block, uncommitted: the guarded block below only selects
        double p5 = p4 + s;                                                // msk.c:82-83
        p5 = wrap_2pi(p5);
        float c5 = (float)((double)c4 + s);                          // msk.c:95
        LEAN_HOLD_STEP5(p5, c5, myp[3 / LPC]);
        const bool fired5 = (double)c5 >= thr;
#ifndef ACG_LEAN_AB_PICK0
        if ((4 % LPC) == g) myp[4 / LPC] = p5;
#endif
        double p6 = p5 + s;
        p6 = wrap_2pi(p6);
        float c6 = (float)((double)c5 + s);
        LEAN_HOLD_STEP(p6, c6, myp[4 / LPC]);
        const bool fired6 = (double)c6 >= thr;
#ifndef ACG_LEAN_AB_PICK0
        if ((5 % LPC) == g) myp[5 / LPC] = p6;
#endif
#endif
        if (n < len && quick) {
#ifdef ACG_LEAN_AB_PICK0
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if ((u % LPC) == g) myp[u / LPC] = pq[u];
#endif
#ifndef ACG_LEAN_AB_SPEC0
#ifdef ACG_LEAN_AB_PICK0
            if ((4 % LPC) == g) myp[4 / LPC] = p5;
            if ((5 % LPC) == g) myp[5 / LPC] = p6;
#endif
            const bool go = !fired5;
            p = go ? p6 : p5;
            L.clk = go ? c6 : c5;
            cnt = go ? 6 : 5;
            fired = go ? fired6 : true;
#else
            p = p4;
            L.clk = c4;
            cnt = 4;
            {
                double pn = p + s;                                         // msk.c:82-83
                pn = wrap_2pi(pn);
                const float cn = (float)((double)L.clk + s);               // msk.c:95
                p = pn;
                L.clk = cn;
                cnt = 5;
                fired = (double)cn >= thr;
                if ((4 % LPC) == g) myp[4 / LPC] = pn;
            }
            {
                const bool go = !fired;
                double pn = p + s;
                pn = wrap_2pi(pn);
                const float cn = (float)((double)L.clk + s);
                if (go) {
                    p = pn;
                    L.clk = cn;
                    cnt = 6;
                    fired = (double)cn >= thr;
                }
                if ((5 % LPC) == g) myp[5 / LPC] = pn;
            }
#endif
        } else if (n < len) {
            double pn = p + s;
            pn = wrap_2pi(pn);
            const float cn = (float)((double)L.clk + s);
            p = pn;
            L.clk = cn;
            cnt = 1;
            fired = (double)cn >= thr;
#ifdef ACG_LEAN_AB_PICK0
            if (g == 0) myp[0] = pn;
#endif
        }
        unsigned int idx_n = idx + (unsigned int)cnt;
        if (idx_n >= FLEN) idx_n -= FLEN;
        clk_f = fired ? (float)((double)L.clk - K_3PI2) : L.clk;           // msk.c:100
        // the mixer's table entries first: kd, q, the LDS address and the read, so that the read's latency runs under the tap phase
        double mr[SPL], mcj[SPL], msj[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) sincos_tab_entry(myp[j], lds.sc, &mr[j], &mcj[j], &msj[j]);
        int o = (int)(MFLTOVER * (div1_rcp((double)clk_f, s) + 0.5));      // msk.c:103
        if (o > MFLTOVER) o = MFLTOVER;
        if (o < 0) o = 0;
        acc = f2v{0.f, 0.f};
        {
            const float* hp = &hs[o];
#pragma unroll
            for (int j = 0; j < FLEN; j += 2) {
                hv2[j / 2].x = hp[j * MFLTOVER];
                hv2[j / 2].y = hp[j + 1 < FLEN ? (j + 1) * MFLTOVER : j * MFLTOVER + 1];
            }
        }
        float2 xo[5];
        {
            const float2* rp0 = &ring[idx_n][slot];
#pragma unroll
            for (int j = 0; j < 5; ++j) xo[j] = rp0[j * CPW];
        }
        // the tap phase and the h[] / old-ring reads stay in FRONT of the mixer: their LDS latency runs under its sin/cos series
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            const int u = g + j * LPC;
            double sn, cs;
#ifdef ACG_LEAN_AB_HORN0
            sincos_tab_rotate(mr[j], mcj[j], msj[j], &sn, &cs);
#else
            sincos_tab_rotate3(mr[j], mcj[j], msj[j], &sn, &cs);
#endif
            const double in = (double)in_cur[j];
            unsigned int k = idx + (unsigned int)u;
            if (k >= FLEN) k -= FLEN;
            if (u >= cnt) k = 2 * FLEN;
            const float2 x = make_float2((float)(in * cs), (float)(in * (-sn)));
            ring[k][slot] = x;
            ring[k + FLEN][slot] = x;
        }
        n += cnt;
        idx = idx_n;
        // the six newest taps, read right behind the ring write (one wave's LDS operations execute in order: the reads see the
        // writes of every lane); the five old taps' arithmetic and the wave-wide test run under their latency
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {
            const float2* rp = &ring[idx_n][slot];
#pragma unroll
            for (int j = 5; j < FLEN; ++j) xs[j - 5] = rp[j * CPW];
        }
        __builtin_amdgcn_sched_barrier(0);
#ifndef ACG_LEAN_AB_WAIT0
        // ONE counted wait for all the old taps use (h[0..5]; the ring entries are older).  Still in flight behind it, in the order
        // of issue: the h[] reads of the newest taps (two pairs and the last), the ring write(s), the three newest-tap reads
        // (pinned: left free, the scheduler moves the wait behind the taps it is for and the compiler's own three come back)
        LEAN_WAIT_LGKM(6 + SPL);
        __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const f2v x = {xo[j].x, xo[j].y};
            acc = acc + MSK_TAP(j, x);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    // ---- the bit decision up to the normalised filter output (msk.c:100-113); for lanes whose bit fired
    float vr, vi, lvl;
    auto decide = [&]() {
        L.clk = clk_f;                                                     // msk.c:100
        {
#pragma unroll
            for (int j = 5; j < FLEN; ++j) {
                const f2v x = {xs[j - 5].x, xs[j - 5].y};
                acc = acc + MSK_TAP(j, x);
            }
        }
        vr = acc.x; vi = acc.y;
        lvl = sqrtf_of_sum_of_squares((double)vr * (double)vr + (double)vi * (double)vi);
        const double d = (double)lvl + 1e-8;
        double qr, qi;
        div2_shared_rcp((double)vr, (double)vi, d, &qr, &qi);
        vr = (float)qr;
        vi = (float)qi;
        L.lvlsum += (double)(lvl * lvl / 4);
    };

    while (__any(n < len)) {
        if (n >= refill_at && n < len) {
            store_block(pend_blk);
            ++pend_blk;
            refill_at += WB;
            fetch_block(pend_blk);
        }
        // ---- a segment: up to SEG periods whose framing waits.  lim = how many bits of this channel may wait: all SEG from a
        // state in which the next possible reset of the loop is at least a byte away, else up to the bit before the byte closes
        const unsigned int aS = (unsigned int)L.astate;
        const bool isW = aS == WSYN, isT = aS == TXT;
        // (nbits outside 1..8 can only come from a state a host wrote with acg_set_state: such a channel takes msk.hip's way)
        const bool safe = (isW | (isT & (L.berr <= MAXPERR) & (L.blen <= 239)) | (aS == CRC1)) & ((unsigned int)(L.nbits - 1) < 8u);
        // (with a bit log: and the segment's records fit -- they are stored without the clamp of the inline path)
        const int lim = (safe & (!LOG || nb + SEG <= a.bit_cap)) ? SEG : L.nbits - 1;
        float2* const brec = LOG ? bits + nb : nullptr;
        const unsigned int S0 = L.S;
        const bool odd0 = (S0 & 1u) != 0;
        const double lvlsum0 = L.lvlsum;
        unsigned int P = 0, N = 0;                 // (vo > 0), (vo < 0) of the segment's bits, oldest in the highest place
        float lvk[SEG];
        int nk[SEG];
#ifndef ACG_LEAN_AB_REC0
        // the segment's bit records: every lane of a group computes the identical record of period k, and lane g KEEPS records g,
        // g + LPC, ... (two selects a period); they leave behind the segment's framing, one store per lane, instead of one store
        // of all 64 lanes per period
        float2 rec[NREC] = {};
#endif
#pragma unroll
        for (int k = 0; k < SEG; ++k) { lvk[k] = 0.f; nk[k] = 0; }
        int c = 0;                                 // bits whose framing waits (wave-uniform)
        bool tail = false;                         // a period's front part is done and its bit decision is not
#pragma unroll
        for (int k = 0; k < SEG; ++k) {
            front();
            // every lane fired a bit and may let its framing wait?  (One lane that cannot: the wave closes the segment and
            // takes this period the way msk.hip does.)  The hint lays "the segment goes on" out as the fall-through.
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(fired && lim > k) != ~0ull, 0)) { tail = true; break; }
            decide();
            // decision + phase detector (msk.c:115-121); S + k is odd where S is odd and k even, ...
            const PhaseDet pd = phase_detect(((k & 1) ? !odd0 : odd0) ? 1u : 0u, vr, vi);          // (only the parity matters)
            const float vo = pd.vo;
            P = shift_in(P, vo > 0);
            N = shift_in(N, vo < 0);
            if constexpr (LOG) {
                // the record under the polarity S + k carries; a ~SYN found when the segment is framed turns the records behind it
                const float sv = __uint_as_float(__float_as_uint(vo) ^ (((S0 + (unsigned int)k) & 2u) << 30));
#ifdef ACG_LEAN_AB_REC0
                brec[k] = make_float2(sv, lvl);
#else
                const bool mine = g == k % LPC;
                rec[k / LPC].x = mine ? sv : rec[k / LPC].x;
                rec[k / LPC].y = mine ? lvl : rec[k / LPC].y;
#endif
            }
            lvk[k] = lvl;
            nk[k] = n;
            L.df = loop_filter(L.df, pd.dphi);
            c = k + 1;
        }
        // ---- framing of the c bits that waited
        if (c > 0) {
            const unsigned int uc = (unsigned int)c;
            const unsigned int Pr = __builtin_bitreverse32(P) >> (32u - uc), Nr = __builtin_bitreverse32(N) >> (32u - uc);   // bit k: k-th bit of the segment
            const unsigned int Mpol = 0x993366CCu >> ((S0 & 3u) * 8u);     // bit k: bit 1 of S0 + k, the polarity putbit() sees (msk.c:122-126)
            const unsigned int B0 = (Mpol & Nr) | (~Mpol & Pr);            // the bits as putbit() takes them
            const unsigned int old = L.outbits;
            const unsigned int W = (B0 << 8) | old;                       // outbits after bit k = (W >> (k + 1)) & 0xff
            const unsigned int m = (unsigned int)L.nbits;                 // the byte closes with bit m - 1
            unsigned int out_end = (W >> uc) & 0xffu;
            const bool reach = m <= uc;
            // WSYN: the first k in [m - 1, c - 1] whose window is SYN (low half) or ~SYN (high half: the complemented stream against SYN)
            const unsigned int V = W >> 1;
            const unsigned int X = ((~V) << 16) | V;
            const unsigned int Y = ~X;
            // a window matches where no place differs: bit k + 7 of `dif` is set if window k differs from SYN = 0001 0110 in some place
            unsigned int dif = X << 7;                                    // place 0 wants 0
            dif |= Y << 6;                                                // place 1 wants 1
            dif |= Y << 5;                                                // place 2 wants 1
            dif |= X << 4;
            dif |= Y << 3;                                                // place 4 wants 1
            dif |= X << 2;
            dif |= X << 1;
            dif |= X;
            const unsigned int valid = reach ? (((1u << uc) - 1u) >> (m - 1u)) << (m - 1u) : 0u;
            const unsigned int hit = ~dif;
            const unsigned int mlo = (hit >> 7) & valid, mhi = (hit >> 23) & valid;
            const unsigned int mm = mlo | mhi;
            // TXT: one plain byte (good parity, no terminator -- tested as `no control character`, the others take the full machine)
            const unsigned int rb = (W >> m) & 0xffu;
            const bool plain = isT & reach & ((__popc(rb) & 1) != 0) & (((rb + 1u) & 0x60u) != 0);
            txt[plain ? L.blen : 255] = (unsigned char)rb;
            L.blen += plain ? 1 : 0;
            int nbits_n = m > uc ? (int)(m - uc) : (isW ? 1 : (int)(m + 8u - uc));
            unsigned int S_n = S0 + uc;
            const int bc0 = L.bitcount;
            L.bitcount = bc0 + c;
            const long long nbt0 = L.nbit_total;
            L.nbit_total = nbt0 + c;
            if constexpr (LOG) nb += c;
            if ((isW & (mm != 0)) | (reach & !isW & !plain)) {
                if (isW) {
                    // sync found at bit k (acars.c:253-263); ~SYN turns the polarity of the bits behind it
                    const unsigned int k = (unsigned int)__builtin_ctz(mm);
                    L.astate = SYN2;
                    nbits_n = 8 - (int)(uc - 1u - k);
                    if ((mhi >> k) & 1u) {
                        S_n = ((S0 + k) ^ 2u) + (uc - k);
                        const unsigned int B1 = (Mpol & Pr) | (~Mpol & Nr);
                        const unsigned int lowm = (2u << k) - 1u;
                        const unsigned int Bx = (B0 & lowm) | (B1 & ~lowm);
                        out_end = (((Bx << 8) | old) >> uc) & 0xffu;
                        if constexpr (LOG) {
#ifdef ACG_LEAN_AB_REC0
                            for (unsigned int j = k + 1u; j < uc; ++j) {
                                const float v = brec[j].x;
                                brec[j].x = -v;
                            }
#else
#pragma unroll
                            for (int q = 0; q < NREC; ++q)
                                if ((unsigned int)(g + q * LPC) > k) rec[q].x = -rec[q].x;
#endif
                        }
                    }
                } else {
                    // a byte that is not plain text closed with bit k: the full machine, with the channel as it was at that bit
                    const unsigned int k = m - 1u;
                    const double lvl_all = L.lvlsum;
                    double ls = lvlsum0;
                    int nn = nk[0];
#pragma unroll
                    for (int i = 0; i < SEG; ++i) {
                        if ((unsigned int)i <= k) ls += (double)(lvk[i] * lvk[i] / 4);
                        if ((unsigned int)i == k) nn = nk[i];
                    }
                    L.lvlsum = ls;
                    L.bitcount = bc0 + (int)k + 1;
                    L.nbit_total = nbt0 + k;
                    L.outbits = rb;
                    L.S = S0 + k;
                    decode_acars(L, a, ch, txt, samp0 + nn - 1, leader, &st->soh32);
                    nbits_n = L.nbits - (int)(uc - 1u - k);
                    L.lvlsum = lvl_all;
                    L.bitcount = bc0 + c;
                    L.nbit_total = nbt0 + c;
                }
            }
#ifndef ACG_LEAN_AB_REC0
            if constexpr (LOG) {
#pragma unroll
                for (int q = 0; q < NREC; ++q)
                    if (g + q * LPC < c) brec[g + q * LPC] = rec[q];
            }
#endif
            L.nbits = nbits_n;
            L.outbits = out_end;
            L.S = S_n;
        }
        // ---- the period that closed the segment, msk.hip's way: framing inline
        if (tail) {
            if (fired) {
                decide();
                L.bitcount += 1;
                const PhaseDet pd = phase_detect(L.S, vr, vi);
                const float sv = __uint_as_float(__float_as_uint(pd.vo) ^ ((L.S & 2u) << 30));   // msk.c:122-126
                if constexpr (LOG) {
                    bits[nb < a.bit_cap ? nb : a.bit_cap - 1] = make_float2(sv, lvl);
                    nb += 1;
                }
                frame_bit<true>(L, sv, a, ch, txt, samp0 + n - 1, leader, &st->soh32);
                L.df = loop_filter(L.df, pd.dphi);
            }
        }
    }

    if (leader) {
        lane_store(st, L, p, idx, samp0, len);
        ring_save<CPW>(st, ring, slot);
        a.nbits_out[ch] = LOG ? nb : (a.bit_append ? a.nbits_out[ch] : 0) + (int)(L.nbit_total - nbt_in);
    }
    publish_queue_length<WPG>(a);
}
