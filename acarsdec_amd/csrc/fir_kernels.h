// fir_kernels.h -- the wave-private streaming down-converter kernels (fir_u8_direct_kernel, fir_s8_direct_kernel,
// fir_fmt_direct_kernel) and the launch helpers of their units.  fir.hip instantiates the u8 I/Q kernels and the front ends' sample
// formats, fir_iq.hip the recordings' formats (complex int8 on the u8 kernels' signed switch, complex float32 on the format
// kernels); a template is compiled where it is launched.  The tile kernels, the fallbacks of every format and window length, are
// fir_tile_kernel.h; what both families reach is fir_common.h.  Not a unit of its own.
#ifndef ACG_FIR_KERNELS_H
#define ACG_FIR_KERNELS_H
#include <hip/hip_runtime.h>
#include <type_traits>
#include "acg_internal.h"
#include "fir_plan.h"
#include "fir_common.h"

// ---------------------------------------------------------------------------------------------------
// Wave-private streaming variant -- the default for whole callbacks at the documented rates
// (rtlMult 160 / 192 / 200, rtl.c:244-262).  What the workgroup-granular kernels (fir_tile_kernel.h) pay for is
// structure, not arithmetic: two barriers per tile, a partial-sum exchange between the four
// waves and a single finishing wave.  Here a wave owns its tiles outright and never talks to another wave:
//   * the input never passes through LDS: a tile (64 windows x 2M bytes = CPR KiB, contiguous in HBM) is
//     read as CPR wave-loads of 1 KiB (16 bytes per lane, non-temporal, one uniform base + lane offset),
//     U loads always in flight per wave, across tile and run boundaries -- the access pattern of a pure
//     streaming reader;
//   * lane L of wave-load q holds 16-byte chunk i = 64 q + L = 8 consecutive complex samples of window
//     i / CPR at column i % CPR.  The taps of that column come from a per-wave LDS copy of the channel's
//     tap table, laid out [4 planes][CPR + 63 columns] with the columns replicated past CPR, so that
//     the lane address is one base + a compile-time offset per q (no per-lane modulo) and the four
//     ds_read_b128 of a step are bank-conflict free;
//   * the 8-sample partial sum (re, im) of every chunk goes to a per-wave LDS array; after the CPR-th load
//     lane = window adds the CPR partials of its window (row stride odd: conflict free), takes |D| and
//     the wave writes 64 consecutive floats of dm.  All 64 lanes of every wave do this (no finishing wave);
//   * work is handed out per WAVE in runs of 2 tiles (one channel) by a sharded ticket dispenser
//     (ACG_DISP_SHARDS counters, each serving a contiguous eighth of the run space in address order;
//     a wave whose shard is exhausted moves on to the next one).  The ticket for the next run is
//     requested a whole tile before it is needed; the next run's taps are fetched during the last tile.
// Summation order: 8 sequential fused multiply-adds per chunk, then CPR sequential adds (the reference
// adds M terms sequentially; its own -Ofast build reassociates, SURVEY 8c: dm within 1e-5 relative).

template <int CPR, int U_ = 0, int B_ = 0>
struct FirD {
    // U staging slots per lane: run position p lives in slot p % U, so U divides the loads of a run.  Loads are
    // issued in bursts of B consecutive wave-loads (B KiB contiguous per wave) every B steps, as the slots of the
    // B positions consumed since the last burst are free again: between U - B and U KiB per wave are in flight.
    static constexpr int U = U_ ? U_ : ((FIRD_R * CPR) % 10 == 0) ? 10 : 12;
    static constexpr int B = B_ ? B_ : U / 2;
    static constexpr int TS = CPR + 63;                                        // tap columns incl. replicas
    static constexpr int PW = (CPR & 1) ? CPR : CPR + 1;                       // partial-sum row stride (odd)
    static constexpr int TAB_BYTES = 4 * TS * 16;
    static constexpr int P_BYTES = 64 * PW * 8;
    static constexpr int WAVE_LDS = TAB_BYTES + P_BYTES;
    static_assert((FIRD_R * CPR) % U == 0 && (FIRD_R * CPR) % B == 0 && B <= U, "slots and bursts must divide the loads per run");
};

typedef unsigned int u4v_t __attribute__((ext_vector_type(4)));

// Raw buffer descriptor over [base, base + bytes): loads beyond `bytes` return 0 without touching memory,
// so "no next run" is a descriptor of 0 bytes instead of a branch around every prefetch.  Loads through a
// descriptor are `buffer_load_dwordx4 v, voff, s[rsrc], soffset offen nt`: one VGPR offset (lane * 16), the
// tile / load position as scalar offset, no vector address arithmetic, the non-temporal bit explicit.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fird_rsrc(const void* base, unsigned int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ u4v_t fird_load(__amdgpu_buffer_rsrc_t r, unsigned int voff, unsigned int soff)
{
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 2 /* nt */);
}

// The sharded ticket dispenser as one wave sees it.  Shard s hands out runs s, s + SHARDS, s + 2 SHARDS, ...: the shards advance
// together, so the whole grid reads ONE front that moves through the input in address order (HBM likes that better than eight
// distant fronts), while the ticket atomics are spread over eight L2 channels.  The first run of wave wg is run wg (static);
// tickets count on from there.  A wave whose shard has run dry moves on to the next one; the last wave to sign off re-arms
// all words, so no memset launch precedes the kernel.
// The members are REFERENCES to the kernel's own values (what the lambdas this replaced captured), and "is there a run?" is
// asked by the caller (`if (run == NONE) run = disp.probe_after(s)`): with values held by copy, or with that test folded into a
// member, the format kernels compile to other text (profiles/LEDGER.md, "Down-converter: one copy of the shared parts").
struct RunDisp {
    static constexpr unsigned int NONE = 0xffffffffu;
    unsigned int* const& ctr;                                       // FirArgs::work_counter
    const unsigned int &nrun, &nwaves;
    const int& lane;
    __device__ unsigned int shard_runs(unsigned int s) const { return (nrun + ACG_DISP_SHARDS - 1 - s) / ACG_DISP_SHARDS; }
    __device__ unsigned int shard_static(unsigned int s) const { return (nwaves + ACG_DISP_SHARDS - 1 - s) / ACG_DISP_SHARDS; }
    __device__ static unsigned int after(unsigned int s) { return (s + 1 == ACG_DISP_SHARDS) ? 0 : s + 1; }
    __device__ unsigned int run_of_ticket(unsigned int s, unsigned int t) const
    {
        const unsigned long long k = (unsigned long long)shard_static(s) + t;
        return k < shard_runs(s) ? (unsigned int)k * ACG_DISP_SHARDS + s : NONE;
    }
    __device__ unsigned int probe(unsigned int& s) const            // synchronous: next run of shard s, else of the following shards
    {
        for (int k = 0; k < ACG_DISP_SHARDS; ++k) {
            unsigned int t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(ctr + s * ACG_DISP_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t = (unsigned int)__builtin_amdgcn_readfirstlane((int)t);
            const unsigned int r = run_of_ticket(s, t);
            if (r != NONE) return r;
            s = after(s);
        }
        return NONE;
    }
    // shard s has run dry: on to the shards after it
    __device__ unsigned int probe_after(unsigned int& s) const
    {
        s = after(s);
        return probe(s);
    }
    __device__ void sign_off() const
    {
        if (lane == 0) {
            const unsigned int d = atomicAdd(ctr + ACG_DISP_SHARDS * ACG_DISP_STRIDE, 1u);
            if (d == nwaves - 1) {                                  // every wave's requests have been answered: re-arm
#pragma unroll
                for (int k = 0; k <= ACG_DISP_SHARDS; ++k)
                    __hip_atomic_store(ctr + k * ACG_DISP_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
};

// (the ticket for the run after the current one is requested by lane 0 a whole tile before it is looked at: ticket_request /
//  ticket_take, fir_common.h; the U loads and the store in flight are all younger than it)

// one tile: CPR steps.  A step is fenced off from its neighbours with scheduling barriers -- left alone, the scheduler
// delays the loads to shorten live ranges (the pipeline then runs dry at the end of a tile) or bunches them up at
// random, and the result changes with every edit.  Inside a step: first the memory instructions whose results are
// needed LATER (every B-th step the burst of B wave-loads U - B positions ahead, the next step's taps from LDS), then
// this step's arithmetic on data that arrived long ago.
// FOLD: sum (x - 127.37)(w) = sum x w - 127.37 (1 + j) sum w.  The second term is a constant of the channel (dc, formed
// when the tap table is loaded), so the eight v_pk_add_f32 per 16 input bytes that subtract 127.37 from every sample
// (a fifth of the loop's vector instructions) become one subtraction per window.  x - 127.37f is exact in f32 either
// way; what changes is the order of the roundings in the sum, at the 1e-7 level of full scale like any re-association
// (rtl.c builds with -Ofast and re-associates itself; the parity bar for dm is 1e-5).
template <int CPR, int UU, int BB, int TILE, bool FOLD, bool WT = false, bool NOMAC = false, bool S8 = false>
__device__ __forceinline__ void fird_tile(u4v_t* st /* [U] */, __amdgpu_buffer_rsrc_t cur, __amdgpu_buffer_rsrc_t nxt,
                                          unsigned int voff, const float4* Tl, f2* Pw, const f2* Pr, float* __restrict__ dm_out, int lane,
                                          f2 dc)
{
    typedef FirD<CPR, UU, BB> F;
    float4 w0 = Tl[0 * F::TS], w1 = Tl[1 * F::TS], w2 = Tl[2 * F::TS], w3 = Tl[3 * F::TS];          // step 0: column of lane 0 is 0
#pragma unroll
    for (int q = 0; q < CPR; ++q) {
        __builtin_amdgcn_sched_barrier(0);
        const int p = TILE * CPR + q;                         // run position consumed by this step
        u4v_t d = st[p % F::U];
        if (S8) d ^= 0x80808080u;                             // int8 -> int8 + 128 as u8: the byte conversions below, 128 folded out
        if (p % F::B == 0) {
#pragma unroll
            for (int b = 0; b < F::B; ++b) {
                const int pos = p + F::U - F::B + b;          // slots of positions p - B .. p - 1 are free
                if (pos < FIRD_R * CPR) st[pos % F::U] = fird_load(cur, voff, (unsigned int)pos * 1024u);
                else st[pos % F::U] = fird_load(nxt, voff, (unsigned int)(pos - FIRD_R * CPR) * 1024u);
            }
        }
        float4 n0 = w0, n1 = w1, n2 = w2, n3 = w3;
        if (q + 1 < CPR) {
            const int c1 = ((q + 1) * 64) % CPR;              // column of lane 0 in the next load (compile time)
            n0 = Tl[0 * F::TS + c1]; n1 = Tl[1 * F::TS + c1]; n2 = Tl[2 * F::TS + c1]; n3 = Tl[3 * F::TS + c1];
        }
        __builtin_amdgcn_sched_barrier(0);
        const float w[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
        f2 accA = {0.f, 0.f};       // (sum tr*wr, sum ti*wi)
        f2 accB = {0.f, 0.f};       // (sum tr*wi, sum ti*wr)
        if (NOMAC) {                // measurement variant 56: the loads are consumed, nothing is converted or multiplied, no tap reads
            accA.x = __uint_as_float((d[0] ^ d[1]) & 0x3fffffffu);
            accB.x = __uint_as_float((d[2] ^ d[3]) & 0x3fffffffu);
        } else
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned int word = d[j >> 1];
            const unsigned int sh = (j & 1) * 16;
            f2 tt;
            tt.x = (float)((word >> sh) & 0xffu);                      // rtl.c:338 (the conversion and the difference are exact in f32)
            tt.y = (float)((word >> (sh + 8)) & 0xffu);                // rtl.c:339
            if (!FOLD) { tt.x -= 127.37f; tt.y -= 127.37f; }
            const f2 wv = {w[2 * j], w[2 * j + 1]};
            const f2 ws = {w[2 * j + 1], w[2 * j]};
            accA = __builtin_elementwise_fma(tt, wv, accA);
            accB = __builtin_elementwise_fma(tt, ws, accB);
        }
        const f2 part = {accA.x - accA.y, accB.x + accB.y};
        if (F::PW == CPR) {
            Pw[q * 64] = part;                                         // chunk i = 64 q + lane, rows of CPR
        } else {
            const unsigned int i = (unsigned int)(q * 64 + lane);
            const unsigned int r = (i * ((65536u + CPR - 1) / CPR)) >> 16;   // i / CPR for i < 64 * CPR <= 2048
            Pw[q * 64 + (int)r] = part;                                // + one pad entry per completed row
        }
        w0 = n0; w1 = n1; w2 = n2; w3 = n3;
    }
    __builtin_amdgcn_sched_barrier(0);
    // lane = window: add the CPR partial sums of the row, |D| (rtl.c:353), 64 consecutive floats
    f2 D = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CPR; ++j) D = D + Pr[j];
    if (FOLD) D = D - dc;
    if (WT) {                                                      // write-through store (the default; 55 = write-back): DESIGN 4
        float* p = dm_out + lane;
        float v = cabs_like_glibc(D.x, D.y);
        if (S8) v *= 1.0f / 128.0f;                                // ACG_FMT_CS8: dm = |D| / 128 (a power of two: exact)
        asm volatile("global_store_dword %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
    } else {
        dm_out[lane] = cabs_like_glibc(D.x, D.y);
    }
}

template <int CPR, int UU, int BB, bool FOLD, bool WT = false, bool NOMAC = false, bool S8 = false>
__device__ __forceinline__ void fird_body(const FirArgs& a, const uint8_t* __restrict__ iq_base, const float* __restrict__ taps_base,
                                          const int* __restrict__ stream_of, float* __restrict__ dm_base)
{
    typedef FirD<CPR, UU, BB> F;
    constexpr unsigned int NONE = RunDisp::NONE;
    // beside demodulator waves (which have slack whenever this kernel is the longer stage) this stream wins the issue
    // arbitration: the demodulator then fills the gaps instead of stretching the bandwidth-bound stage
    if (a.high_prio) __builtin_amdgcn_s_setprio(2);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char* my = fir_smem + wave * F::WAVE_LDS;
    float4* T = (float4*)my;
    f2* P = (f2*)(my + F::TAB_BYTES);
    const float4* Tl = T + lane;                                   // + (plane * TS + c0(q)) compile-time slots
    f2* Pw = P + lane;                                             // + 64 q entries
    const f2* Pr = P + lane * F::PW;

    // A run is `pairs` consecutive two-tile bodies of one channel (launcher: 1 for small launches, up to 8 for large
    // ones, so that every wave still gets ~32 runs): the per-run work (ticket, row lookup, tap table) is paid once per run.
    const unsigned int pairs = (unsigned int)a.run_pairs;
    const unsigned int ntile = (unsigned int)a.nwin / ACG_TILE_WIN;                 // whole tiles only (launcher)
    const unsigned int runs_per_ch = ntile / (FIRD_R * pairs);                      // ntile % (FIRD_R * pairs) == 0 (launcher)
    const unsigned int nrun = (unsigned int)a.nch * runs_per_ch;
    const unsigned int wpg = blockDim.x >> 6;                                       // the waves of a workgroup never talk to each other
    const unsigned int nwaves = gridDim.x * wpg;
    const unsigned int wg = blockIdx.x * wpg + (unsigned int)wave;
    unsigned int* ctr = a.work_counter;
    constexpr unsigned int tile_bytes = (unsigned int)CPR * 1024u;
    constexpr unsigned int run_bytes = FIRD_R * tile_bytes;                         // bytes of one two-tile body
    const unsigned int voff = (unsigned int)lane << 4;
    const int nck = a.ntaps_pad >> 3;                                               // tap columns that carry taps

    const RunDisp disp = {ctr, nrun, nwaves, lane};
    auto run_base = [&](unsigned int run, unsigned int& ch, unsigned int& t0) -> const uint8_t* {
        ch = run / runs_per_ch;
        t0 = (run - ch * runs_per_ch) * FIRD_R * pairs;
        const size_t row = (size_t)(a.stream_identity ? (int)ch : stream_of[ch]) * a.pitch;
        return iq_base + row + (size_t)t0 * tile_bytes;
    };
    // taps of channel ch, column = lane (64 bytes); the values are not looked at before write_taps, so the
    // loads stay in flight under the last tile of the run
    auto fetch_taps = [&](unsigned int ch, float4 (&tp)[4]) {
        const float4* src = (const float4*)(taps_base + (size_t)ch * a.ntaps_pad * 2) + (lane < nck ? lane : 0) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) tp[k] = src[k];
    };
    f2 dc = {0.f, 0.f};                                             // 127.37 (1 + j) sum w of the current run's channel
    auto write_taps = [&](const float4 (&tp)[4]) {
        const bool on = lane < nck;                                 // columns beyond the last tap: zero
        if (FOLD) {
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) { sr += tp[k].x + tp[k].z; si += tp[k].y + tp[k].w; }
            sr = on ? sr : 0.f;
            si = on ? si : 0.f;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) { sr += __shfl_xor(sr, m, 64); si += __shfl_xor(si, m, 64); }
            dc.x = (S8 ? 128.0f : 127.37f) * (sr - si);
            dc.y = (S8 ? 128.0f : 127.37f) * (sr + si);
        }
#pragma unroll
        for (int rep = 0; rep * CPR < F::TS; ++rep) {
            const int u = lane + rep * CPR;
            if (lane < CPR && u < F::TS) {
#pragma unroll
                for (int k = 0; k < 4; ++k) T[k * F::TS + u] = on ? tp[k] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };

    unsigned int s = wg % ACG_DISP_SHARDS;
    unsigned int run = wg < nrun ? wg : NONE;                       // the first run of wave wg is run wg
    if (run == NONE) run = disp.probe_after(s);                     // tiny launches: fewer runs than waves
    if (run == NONE) { disp.sign_off(); return; }

    unsigned int ch, t0;
    const uint8_t* base = run_base(run, ch, t0);
    {
        float4 tp[4];
        fetch_taps(ch, tp);
        write_taps(tp);
    }
    __amdgpu_buffer_rsrc_t cur = fird_rsrc(base, run_bytes);
    u4v_t st[F::U];
#pragma unroll
    for (int i = 0; i < F::U - F::B; ++i) {                         // step 0 issues the burst U - B .. U - 1 itself
        st[i] = fird_load(cur, voff, (unsigned int)i * 1024u);
        __builtin_amdgcn_sched_barrier(0);                          // keep the loads in issue order (the waits count on it)
    }

    for (;;) {
        // ask for the run after this one now; the answer is looked at in the run's last body, at least a tile later
        unsigned int tk;
        if (lane == 0) ticket_request(ctr + s * ACG_DISP_STRIDE, tk);
        float* __restrict__ dm_out = dm_base + (size_t)ch * a.dm_pitch + (size_t)t0 * ACG_TILE_WIN;
        static_assert(FIRD_R == 2, "a body is unrolled by hand: first tile, second tile");
        bool has_next = true;
        unsigned int nrun_ = NONE, nch_ = ch, nt0 = t0;
        float4 tp[4];
        for (unsigned int j = 0; j < pairs; ++j) {
            fird_tile<CPR, UU, BB, 0, FOLD, WT, NOMAC, S8>(st, cur, cur, voff, Tl, Pw, Pr, dm_out, lane, dc);
            // second tile of the body: where does the stream go next?
            const uint8_t* nbase = base + run_bytes;                // the next body of this run ...
            if (j + 1 == pairs) {                                   // ... or the first body of the next run
                // (U loads and a store are in flight, all younger than the ticket)
                nrun_ = disp.run_of_ticket(s, (unsigned int)__builtin_amdgcn_readfirstlane((int)ticket_take<F::U + 1>(tk)));
                if (nrun_ == NONE) nrun_ = disp.probe_after(s);
                has_next = nrun_ != NONE;
                nbase = base;
                if (has_next) nbase = run_base(nrun_, nch_, nt0);
                fetch_taps(nch_, tp);
            }
            const __amdgpu_buffer_rsrc_t nxt = fird_rsrc(nbase, has_next ? run_bytes : 0u);
            fird_tile<CPR, UU, BB, 1, FOLD, WT, NOMAC, S8>(st, cur, nxt, voff, Tl, Pw, Pr, dm_out + ACG_TILE_WIN, lane, dc);
            dm_out += FIRD_R * ACG_TILE_WIN;
            base = nbase;
            cur = nxt;
        }
        if (!has_next) break;
        write_taps(tp);
        run = nrun_;
        ch = nch_;
        t0 = nt0;
    }
    disp.sign_off();
}

template <int CPR, int UU = 0, int BB = 0, bool FOLD = true, bool WT = false, bool NOMAC = false>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_u8_direct_kernel(const FirArgs a,
                                                                    const uint8_t* __restrict__ iq_base,
                                                                    const float* __restrict__ taps_base,
                                                                    const int* __restrict__ stream_of,
                                                                    float* __restrict__ dm_base)
{
    fird_body<CPR, UU, BB, FOLD, WT, NOMAC>(a, iq_base, taps_base, stream_of, dm_base);
}

// ACG_FMT_CS8 (interleaved int8 I,Q: SigMF ci8, HackRF), one stream per channel: the same kernel with the signed switch.  A byte
// xor 0x80 is the sample + 128 as u8, so the loop is the u8 loop behind four v_xor per 16 bytes, the constant folded out of the
// sum is 128 (1 + j) sum w, and |D| leaves scaled by 1/128.  Write-through stores, as the u8 default.
template <int CPR>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_s8_direct_kernel(const FirArgs a,
                                                                    const uint8_t* __restrict__ iq_base,
                                                                    const float* __restrict__ taps_base,
                                                                    const int* __restrict__ stream_of,
                                                                    float* __restrict__ dm_base)
{
    fird_body<CPR, 0, 0, true, true, false, true>(a, iq_base, taps_base, stream_of, dm_base);
}

// ---------------------------------------------------------------------------------------------------
// The wave-private streaming kernel for the other front ends' sample formats (4 bytes per sample; split planes: two
// 16-byte chunks -- 8 I and 8 Q samples -- per step).  Same structure as fir_u8_direct_kernel: the input never passes
// through LDS, wave-loads are issued in bursts U - B positions ahead, the taps of a lane's column come from a per-wave
// LDS copy of the channel's tap table with replicated columns, per-chunk partial sums are transposed through a per-wave
// LDS array, work is handed out per wave by the sharded ticket dispenser.  What the format changes:
//   * a window is CPR chunks per plane (M = 200 interleaved int16 or real f32: 50; Airspy at 6 / 10 Msps: 120 / 200),
//     so a tile is W = 32, 16 or 8 windows (W * CPR chunks = a whole number of wave-loads) and S = 64 / W adjacent lanes
//     add up the partial sums of one window -- E = CPR / S consecutive entries each -- and meet through S - 1 lane
//     exchanges;
//   * the arithmetic per chunk: 4 complex samples (CS16), 4 real samples against complex taps (F32R: half the
//     multiply-adds), 8 complex samples from two planes (SPLIT), 2 complex f32 samples (CF32: a window of M = 160 / 192 / 200 is
//     CPR = 80 / 96 / 100 chunks, W = 16, so S = 4 lanes add E = 20 / 24 / 25 partial sums each and a wave needs 12.7 / 15.0 /
//     15.0 KiB of LDS: eight waves fit a CU; with W = 32 the partial sums alone were 26 KiB per wave); the power-of-two output
//     scale is applied to |D|.
template <int FMT, int CPR, int W>
struct FirX {
    static constexpr int NPL = (FMT == FMT_SPLIT) ? 4 : (FMT == FMT_CF32) ? 1 : 2;     // 16-byte tap planes per column (8, 2 or 4 taps)
    static constexpr int SPC = (FMT == FMT_SPLIT) ? 8 : (FMT == FMT_CF32) ? 2 : 4;     // samples (taps) per column
    static constexpr int NLD = (FMT == FMT_SPLIT) ? 2 : 1;             // wave-loads per step
    static constexpr int LT = W * CPR / 64;                            // steps per tile
    static constexpr int S = 64 / W;                                   // lanes per window in the reduction
    static constexpr int E = CPR / S;                                  // partial sums per lane
    static constexpr int EP = (E & 1) ? E : E + 1;                     // odd lane stride: conflict-free reads
    static constexpr int LR = FIRD_R * LT;                             // steps per run
    static constexpr int U = (LR % 10 == 0) ? 10 : 12;
    static constexpr int B = U / 2;
    static constexpr int TS = CPR + 63;
    static constexpr int NPASS = (CPR + 63) / 64;                      // tap-table columns per lane
    static constexpr int TAB_BYTES = NPL * TS * 16;
    static constexpr int P_BYTES = 64 * EP * 8;
    static constexpr int WAVE_LDS = TAB_BYTES + P_BYTES;
    static constexpr unsigned int TILE_BYTES = (unsigned int)W * CPR * 16u;     // per plane
    static_assert((W * CPR) % 64 == 0 && CPR % S == 0 && LR % U == 0 && LR % B == 0 && B <= U, "tile geometry");
};

template <int FMT, int CPR, int W, int TILE>
__device__ __forceinline__ void firx_tile(u4v_t* st /* [NLD][U] */, __amdgpu_buffer_rsrc_t cur0, __amdgpu_buffer_rsrc_t cur1,
                                          __amdgpu_buffer_rsrc_t nxt0, __amdgpu_buffer_rsrc_t nxt1, unsigned int voff, const float4* Tl,
                                          f2* Pw, const f2* Pr, float* __restrict__ dm_out, int lane, float out_scale)
{
    typedef FirX<FMT, CPR, W> F;
    float4 w[F::NPL], nw[F::NPL];
#pragma unroll
    for (int k = 0; k < F::NPL; ++k) w[k] = Tl[k * F::TS];                 // step 0: column of lane 0 is 0
#pragma unroll
    for (int q = 0; q < F::LT; ++q) {
        __builtin_amdgcn_sched_barrier(0);
        const int p = TILE * F::LT + q;                                    // run position consumed by this step
        u4v_t d[F::NLD];
#pragma unroll
        for (int l = 0; l < F::NLD; ++l) d[l] = st[l * F::U + p % F::U];
        if (p % F::B == 0) {
#pragma unroll
            for (int b = 0; b < F::B; ++b) {
                const int pos = p + F::U - F::B + b;
                if (pos < F::LR) {
                    st[pos % F::U] = fird_load(cur0, voff, (unsigned int)pos * 1024u);
                    if (F::NLD == 2) st[F::U + pos % F::U] = fird_load(cur1, voff, (unsigned int)pos * 1024u);
                } else {
                    st[pos % F::U] = fird_load(nxt0, voff, (unsigned int)(pos - F::LR) * 1024u);
                    if (F::NLD == 2) st[F::U + pos % F::U] = fird_load(nxt1, voff, (unsigned int)(pos - F::LR) * 1024u);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < F::NPL; ++k) nw[k] = w[k];
        if (q + 1 < F::LT) {
            const int c1 = ((q + 1) * 64) % CPR;
#pragma unroll
            for (int k = 0; k < F::NPL; ++k) nw[k] = Tl[k * F::TS + c1];
        }
        __builtin_amdgcn_sched_barrier(0);
        float wf[4 * F::NPL];
#pragma unroll
        for (int k = 0; k < F::NPL; ++k) { wf[4 * k] = w[k].x; wf[4 * k + 1] = w[k].y; wf[4 * k + 2] = w[k].z; wf[4 * k + 3] = w[k].w; }
        f2 accA = {0.f, 0.f}, accB = {0.f, 0.f};
        f2 part;
        if (FMT == FMT_CS16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f2 tt;
                tt.x = (float)(short)(d[0][j] & 0xffffu);                  // soapy.c:238
                tt.y = (float)((int)d[0][j] >> 16);                        // soapy.c:239
                const f2 wv = {wf[2 * j], wf[2 * j + 1]};
                const f2 ws = {wf[2 * j + 1], wf[2 * j]};
                accA = __builtin_elementwise_fma(tt, wv, accA);
                accB = __builtin_elementwise_fma(tt, ws, accB);
            }
            part = {accA.x - accA.y, accB.x + accB.y};
        } else if (FMT == FMT_SPLIT) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned int wi_ = d[0][j >> 1], wq_ = d[F::NLD - 1][j >> 1];
                f2 tt;
                tt.x = (j & 1) ? (float)((int)wi_ >> 16) : (float)(short)(wi_ & 0xffffu);     // sdrplay.c:219
                tt.y = (j & 1) ? (float)((int)wq_ >> 16) : (float)(short)(wq_ & 0xffffu);     // sdrplay.c:220
                const f2 wv = {wf[2 * j], wf[2 * j + 1]};
                const f2 ws = {wf[2 * j + 1], wf[2 * j]};
                accA = __builtin_elementwise_fma(tt, wv, accA);
                accB = __builtin_elementwise_fma(tt, ws, accB);
            }
            part = {accA.x - accA.y, accB.x + accB.y};
        } else if (FMT == FMT_CF32) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f2 tt = {__uint_as_float(d[0][2 * j]), __uint_as_float(d[0][2 * j + 1])};   // soapy.c:238-239 without the conversion
                const f2 wv = {wf[2 * j], wf[2 * j + 1]};
                const f2 ws = {wf[2 * j + 1], wf[2 * j]};
                accA = __builtin_elementwise_fma(tt, wv, accA);
                accB = __builtin_elementwise_fma(tt, ws, accB);
            }
            part = {accA.x - accA.y, accB.x + accB.y};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float sv = __uint_as_float(d[0][j]);
                const f2 tt = {sv, sv};                                    // air.c:315-316: wf[i] * S
                const f2 wv = {wf[2 * j], wf[2 * j + 1]};
                accA = __builtin_elementwise_fma(tt, wv, accA);
            }
            part = accA;
        }
        if (F::EP == F::E) {
            Pw[q * 64] = part;
        } else {
            const unsigned int i = (unsigned int)(q * 64 + lane);
            const unsigned int r = (i * ((65536u + F::E - 1) / F::E)) >> 16;           // i / E for i < 64 * E <= 4096
            Pw[q * 64 + (int)r] = part;
        }
#pragma unroll
        for (int k = 0; k < F::NPL; ++k) w[k] = nw[k];
    }
    __builtin_amdgcn_sched_barrier(0);
    // lane l adds entries l * E .. l * E + E - 1 (window l / S, its (l % S)-th part); S adjacent lanes meet
    f2 D = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < F::E; ++j) D = D + Pr[j];
#pragma unroll
    for (int m = 1; m < F::S; m <<= 1) {
        D.x += __shfl_xor(D.x, m);
        D.y += __shfl_xor(D.y, m);
    }
    // power-of-two output scale (1/32768 soapy.c:241, 1/4 sdrplay.c:225): exact, commutes with cabsf
    // (write-through like the u8 kernel's: beside the streaming reads a dirty line that waits in L2 costs more than one that
    //  leaves at once)
    if (lane % F::S == 0) {
        float* p = dm_out + lane / F::S;
        const float v = cabs_like_glibc(D.x, D.y) * out_scale;
        asm volatile("global_store_dword %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
    }
}

template <int FMT, int CPR, int W>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_fmt_direct_kernel(const FirArgs a, const uint8_t* __restrict__ in_base,
                                                                     const float* __restrict__ taps_base,
                                                                     const int* __restrict__ stream_of, float* __restrict__ dm_base)
{
    typedef FirX<FMT, CPR, W> F;
    constexpr unsigned int NONE = RunDisp::NONE;
    if (a.high_prio) __builtin_amdgcn_s_setprio(2);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char* my = fir_smem + wave * F::WAVE_LDS;
    float4* T = (float4*)my;
    f2* P = (f2*)(my + F::TAB_BYTES);
    const float4* Tl = T + lane;
    f2* Pw = P + lane;
    const f2* Pr = P + lane * F::EP;

    // a run = `pairs` consecutive two-tile bodies of one channel (launcher: as many as leave every wave ~32 runs), so that the
    // ticket, the row lookup and the tap table are paid once per run -- as in fir_u8_direct_kernel
    const unsigned int pairs = (unsigned int)a.run_pairs;
    const unsigned int ntile = (unsigned int)a.nwin / W;                            // whole tiles only (launcher)
    const unsigned int runs_per_ch = ntile / (FIRD_R * pairs);
    const unsigned int nrun = (unsigned int)a.nch * runs_per_ch;
    const unsigned int wpg = blockDim.x >> 6;                                       // the waves of a workgroup never talk to each other
    const unsigned int nwaves = gridDim.x * wpg;
    const unsigned int wg = blockIdx.x * wpg + (unsigned int)wave;
    unsigned int* ctr = a.work_counter;
    constexpr unsigned int run_bytes = FIRD_R * F::TILE_BYTES;
    const unsigned int voff = (unsigned int)lane << 4;
    const int nck = a.ntaps_pad / F::SPC;                                           // tap columns that carry taps

    const RunDisp disp = {ctr, nrun, nwaves, lane};
    auto run_base = [&](unsigned int run, unsigned int& ch, unsigned int& t0) -> const uint8_t* {
        ch = run / runs_per_ch;
        t0 = (run - ch * runs_per_ch) * FIRD_R * pairs;
        return in_base + (size_t)(a.stream_identity ? (int)ch : stream_of[ch]) * a.pitch + (size_t)t0 * F::TILE_BYTES;
    };
    // taps of channel ch: lane takes columns lane, lane + 64, ... (16 * NPL bytes each)
    auto fetch_taps = [&](unsigned int ch, float4 (&tp)[F::NPASS][F::NPL]) {
#pragma unroll
        for (int ps = 0; ps < F::NPASS; ++ps) {
            const int col = lane + 64 * ps;
            const float4* src = (const float4*)(taps_base + (size_t)ch * a.ntaps_pad * 2) + (col < nck ? col : 0) * F::NPL;
#pragma unroll
            for (int k = 0; k < F::NPL; ++k) tp[ps][k] = src[k];
        }
    };
    auto write_taps = [&](const float4 (&tp)[F::NPASS][F::NPL]) {
#pragma unroll
        for (int ps = 0; ps < F::NPASS; ++ps) {
            const int col = lane + 64 * ps;
            const bool on = col < nck;
#pragma unroll
            for (int rep = 0; rep * CPR < F::TS; ++rep) {
                const int u = col + rep * CPR;
                if (col < CPR && u < F::TS) {
#pragma unroll
                    for (int k = 0; k < F::NPL; ++k) T[k * F::TS + u] = on ? tp[ps][k] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
    };

    unsigned int s = wg % ACG_DISP_SHARDS;
    unsigned int run = wg < nrun ? wg : NONE;                       // the first run of wave wg is run wg
    if (run == NONE) run = disp.probe_after(s);                     // tiny launches: fewer runs than waves
    if (run == NONE) { disp.sign_off(); return; }

    unsigned int ch, t0;
    const uint8_t* base = run_base(run, ch, t0);
    {
        float4 tp[F::NPASS][F::NPL];
        fetch_taps(ch, tp);
        write_taps(tp);
    }
    __amdgpu_buffer_rsrc_t cur0 = fird_rsrc(base, run_bytes);
    __amdgpu_buffer_rsrc_t cur1 = fird_rsrc(base + (F::NLD == 2 ? a.plane : 0), run_bytes);
    u4v_t st[F::NLD * F::U];
#pragma unroll
    for (int i = 0; i < F::U - F::B; ++i) {
        st[i] = fird_load(cur0, voff, (unsigned int)i * 1024u);
        if (F::NLD == 2) st[F::U + i] = fird_load(cur1, voff, (unsigned int)i * 1024u);
        __builtin_amdgcn_sched_barrier(0);
    }

    for (;;) {
        unsigned int tk;
        if (lane == 0) ticket_request(ctr + s * ACG_DISP_STRIDE, tk);
        float* __restrict__ dm_out = dm_base + (size_t)ch * a.dm_pitch + (size_t)t0 * W;
        static_assert(FIRD_R == 2, "a body is unrolled by hand: first tile, second tile");
        bool has_next = true;
        unsigned int nrun_ = NONE, nch_ = ch, nt0 = t0;
        float4 tp[F::NPASS][F::NPL];
        for (unsigned int j = 0; j < pairs; ++j) {
            firx_tile<FMT, CPR, W, 0>(st, cur0, cur1, cur0, cur1, voff, Tl, Pw, Pr, dm_out, lane, a.out_scale);
            // second tile of the body: where does the stream go next -- the next body of this run, or the next run's first
            const uint8_t* nbase = base + run_bytes;
            if (j + 1 == pairs) {
                nrun_ = disp.run_of_ticket(s, (unsigned int)__builtin_amdgcn_readfirstlane((int)ticket_take<F::NLD * F::U + 1>(tk)));
                if (nrun_ == NONE) nrun_ = disp.probe_after(s);
                has_next = nrun_ != NONE;
                nbase = base;
                if (has_next) nbase = run_base(nrun_, nch_, nt0);
                fetch_taps(nch_, tp);
            }
            const __amdgpu_buffer_rsrc_t nxt0 = fird_rsrc(nbase, has_next ? run_bytes : 0u);
            const __amdgpu_buffer_rsrc_t nxt1 = fird_rsrc(nbase + (F::NLD == 2 ? a.plane : 0), has_next ? run_bytes : 0u);
            firx_tile<FMT, CPR, W, 1>(st, cur0, cur1, nxt0, nxt1, voff, Tl, Pw, Pr, dm_out + W, lane, a.out_scale);
            dm_out += FIRD_R * W;
            base = nbase;
            cur0 = nxt0;
            cur1 = nxt1;
        }
        if (!has_next) break;
        write_taps(tp);
        run = nrun_;
        ch = nch_;
        t0 = nt0;
    }
    disp.sign_off();
}

// ---- launch helpers ----------------------------------------------------------------------------------------------------
// a wave-private kernel's launch: the plan's shape (fir_plan.h), its run length in the arguments
typedef void (*FirWaveKernel)(const FirArgs, const uint8_t*, const float*, const int*, float*);
static inline int launch_planned(FirWaveKernel kernel, const FirWavePlan& p, const FirArgs& a, hipStream_t stream)
{
    FirArgs b = a;
    b.run_pairs = p.pairs;
    FIR_LAUNCH(kernel, dim3((unsigned int)p.grid), dim3(64 * p.wpg), p.lds, stream, b, a.iq, a.taps, a.stream_of, a.dm);
    return (int)hipGetLastError();
}

template <int FMT, int CPR, int W>
static int launch_fmt_direct(const FirArgs* a, int num_cu, hipStream_t stream)
{
    const FirWavePlan p = acg_fir_wave_plan(a, num_cu, FirX<FMT, CPR, W>::WAVE_LDS, W, 8);
    if (p.fit < 1) return (int)hipErrorInvalidValue;
    return launch_planned(fir_fmt_direct_kernel<FMT, CPR, W>, p, *a, stream);
}

// the window lengths fir_u8_direct_kernel and fir_s8_direct_kernel are instantiated for: 16-byte chunks per window (rtlMult 160 / 192 / 200)
#define FIRD_LIST(X) X(20) X(24) X(25)
// the instantiations of fir_fmt_direct_kernel: (format, chunks per window and plane, windows per tile)
#define FIRX_LIST(X) \
    X(FMT_CS16, 40, 32) X(FMT_CS16, 48, 32) X(FMT_CS16, 50, 32) \
    X(FMT_F32R, 50, 32) X(FMT_F32R, 60, 16) X(FMT_F32R, 120, 8) X(FMT_F32R, 200, 8) \
    X(FMT_SPLIT, 20, 64)
// ... and the recordings' (fir_iq.hip launches these)
#define FIRX_LIST_IQ(X) X(FMT_CF32, 80, 16) X(FMT_CF32, 96, 16) X(FMT_CF32, 100, 16)

#endif /* ACG_FIR_KERNELS_H */
