// fir_tile_kernel.h -- the tile family of down-converter kernels: fir_u8_persist_kernel, fir_u8_shared_kernel and fir_fmt_kernel here,
// fir_rate_kernel and fir_long_kernel on top of it (fir_grid_kernel.h), the lab's fir_u8_tile_kernel and fir_u8_dma_kernel.  One
// design: a tile of ACG_TILE_WIN windows goes through LDS one padded row per window (the stride an odd number of 16-byte slots, so
// that "lane = window" ds_read_b128 reads are bank-conflict free), lane = window, the four waves split the taps -- wave-uniform,
// so they come in through scalar loads --, the partial sums meet in LDS, and the next tile is fetched into staging registers while
// this one is computed (issue early, write late).  The parts are written once, here; where a kernel's own rule is needed (which
// stream a row comes from, where a chunk lies) it is handed in as a functor.  A kernel's body is its own arithmetic plus calls.
// THE ORDER OF ADDITIONS IS A CONTRACT: the shared-stream kernel gives the bits of the one-channel kernel and the host feed's pieces
// the bits of one device call (tests/test_gpu_tile_pins.py); it is tile_mac's and tile_wave_sum's.
// A template is compiled where it is launched (fir.hip, fir_iq.hip).  Not a unit of its own.
#ifndef ACG_FIR_TILE_KERNEL_H
#define ACG_FIR_TILE_KERNEL_H
#include <hip/hip_runtime.h>
#include <type_traits>
#include "acg_internal.h"
#include "fir_plan.h"
#include "fir_common.h"

#define FIR_MAXLD 10   // 64 rows * 640 B (M=320) / 16 B / 256 threads
#define FIR_RUN 4      // tiles per dynamically scheduled run (>= 2)
#define FIR_KC 8       // channels of one stream per unit of the shared-stream kernel
#define FMT_MAXLD 14   // 64 rows * 52 chunks (one slice) / 256 threads

typedef unsigned int tile_u4v __attribute__((ext_vector_type(4)));

// ---- LDS: one size per kernel, its launcher's and its own (s_next is the last 16 bytes) ----------------------------------
// tile rows, [4 waves][64] partial sums, the published run id
__host__ __device__ static inline size_t fir_persist_lds(const FirArgs& a) { return ACG_TILE_WIN * a.row_stride + 4 * 64 * sizeof(float4) + 16; }
// tile rows, [4 channels][4 waves][64] partial sums, the published run id
__host__ __device__ static inline size_t fir_shared_lds(const FirArgs& a) { return ACG_TILE_WIN * a.row_stride + 16 * 64 * sizeof(float4) + 16; }
// tile rows (one slice), [4 waves][64] partial sums
__host__ __device__ static inline size_t fir_fmt_lds(const FirArgs& a) { return ACG_TILE_WIN * a.row_stride + 4 * 64 * sizeof(float4); }

// ---- who am I ---------------------------------------------------------------------------------------------------------------
struct TileIds {
    int tid, lane, wave;            // wave: uniform
    __device__ __forceinline__ TileIds()
    {
        tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    }
};

// load slot c of a tile (16-byte chunks, row after row of cpr) -> its row and its chunk in the row; magic: FirArgs::cpr_magic
__device__ __forceinline__ void tile_slot(int c, unsigned int magic, int cpr, int& r, int& col)
{
    r = (int)(((unsigned int)c * magic) >> 20);
    col = c - r * cpr;
}

// n inner steps split over the 4 waves: wave takes [c0, c1)
__device__ __forceinline__ void tile_wave_steps(int n, int wave, int& c0, int& c1)
{
    c0 = n * wave / 4;
    c1 = n * (wave + 1) / 4;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------
// The static contiguous share of G units (a unit: (channel, tile) or (group, tile); the walk does not care) that this workgroup
// takes, so that all workgroups finish together.
__device__ __forceinline__ void tile_static_share(long long G, long long& g0, long long& g1)
{
    g0 = G * blockIdx.x / gridDim.x;
    g1 = G * (blockIdx.x + 1) / gridDim.x;
}

// A static share walked unit by unit, slices innermost: (unit u, tile t, slice k) in LDS, its successor being fetched
// (fir_fmt_kernel's walk; GridWalk of fir_grid_kernel.h spells the same six lines out, see there).
struct SliceWalk : TileIds {
    int ntile;
    const int& kseg;                // the launch's slices per tile, read where it is used
    long long u1;                   // the rounds of this workgroup (units x slices); none: the loop does not run
    int ch, t, k;                   // the unit in LDS
    int nch, nt, nk;                // its successor, the unit being fetched

    // tile_out: outputs per tile
    __device__ __forceinline__ SliceWalk(int nunits, int nwin, int tile_out, const int& kseg_) : kseg(kseg_)
    {
        ntile = (nwin + tile_out - 1) / tile_out;
        long long g0, g1;
        tile_static_share((long long)nunits * ntile, g0, g1);
        u1 = (g1 - g0) * kseg;
        ch = (int)(g0 / ntile);
        t = (int)(g0 - (long long)ch * ntile);
        k = 0;
    }
    // the successor of the unit in LDS (!live: the first unit itself); true: it begins another tile
    __device__ __forceinline__ bool successor(bool live)
    {
        nch = ch, nt = t, nk = live ? k + 1 : 0;
        if (!live || nk != kseg) return false;
        nk = 0;
        if (++nt == ntile) { nt = 0; ++nch; }
        return true;
    }
    __device__ __forceinline__ void advance() { ch = nch, t = nt, k = nk; }
};

// The walk of fir_u8_persist_kernel, fir_u8_shared_kernel and the lab's fir_u8_dma_kernel over G = nunits x tiles.  DYN: runs of
// FIR_RUN tiles handed out by a ticket dispenser, so that workgroups slowed by co-running demodulator waves simply take fewer runs
// instead of stretching the kernel's tail; else one static share.
// The dispenser is two words, {tickets handed out, workgroups finished}, both zero between launches: run ids are gridDim.x + ticket
// (the first run of a workgroup is its own id), and the last workgroup to leave re-arms the pair, so no memset launch precedes the
// kernel.  Thread 0 asks for the next run on a run's first tile (request), publishes the answer through LDS at a barrier one tile
// later (publish) and the workgroup reads it when the run's last tile prefetches across the run boundary (successor).
// The position g of the unit in LDS is the kernel's own loop variable (`for (long long g = w.g0;;)`), handed to the members: held
// as a member beside g0, fir_u8_persist_kernel compiles to 5 VGPRs and 5 to 7 spilled SGPRs more and loses a wave per SIMD
// (profiles/LEDGER.md, "Tile down-converters on one skeleton").  For the same reason a kernel asks none() before it looks at
// anything else of its arguments: what is loaded ahead of that exit stays live across start's divisions.
template <bool DYN>
struct RunWalk {
    unsigned int* counter;          // FirArgs::work_counter
    int* s_next;                    // LDS: the id of the next run
    int ntile;
    long long G, nrun;
    long long g0, g1;               // the run [g0, g1) of the unit in LDS
    int u, t;                       // ... as (unit, tile)
    long long ng, ng0, ng1;         // the successor and its run
    int nu, nt;
    bool more;
    unsigned int pending;           // thread 0: the ticket in flight

    __device__ __forceinline__ RunWalk(int nunits, int nwin)
    {
        ntile = (nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
        G = (long long)nunits * ntile;
        nrun = (G + FIR_RUN - 1) / FIR_RUN;
        if (DYN) {
            g0 = (long long)blockIdx.x * FIR_RUN;       // first run: own id (the counter starts at gridDim.x)
            g1 = g0 + FIR_RUN < G ? g0 + FIR_RUN : G;
        } else {
            tile_static_share(G, g0, g1);
        }
    }
    // this workgroup has no unit: the kernel returns at once
    __device__ __forceinline__ bool none() const { return g0 >= g1; }
    // the first unit.  s_next_: four bytes of LDS for the id of the next run
    __device__ __forceinline__ void start(unsigned int* counter_, int* s_next_)
    {
        counter = counter_;
        s_next = s_next_;
        u = (int)(g0 / ntile);
        t = (int)(g0 - (long long)u * ntile);
        pending = 0;
    }
    __device__ __forceinline__ void request(int tid, long long g)
    {
        if (DYN && g == g0 && tid == 0) ticket_request(counter, pending);
    }
    // at: the unit at whose barrier the answer is published (a run's first tile, or the one behind it)
    __device__ __forceinline__ void publish(int tid, long long g, long long at)
    {
        if (DYN && g == at && tid == 0) *s_next = (int)(gridDim.x + ticket_take<0>(pending));
    }
    // where does the stream go next?  true: there is a successor (nu, nt)
    __device__ __forceinline__ bool successor(long long g)
    {
        nu = u, nt = t + 1;
        if (nt == ntile) { nt = 0; ++nu; }
        more = g + 1 < g1;
        ng0 = g0, ng1 = g1, ng = g + 1;
        if (DYN && !more) {
            // (runs are >= 2 tiles except possibly the very last one, which has no successor anyway)
            const long long nr = (g1 - g0 >= 2) ? (long long)*s_next : nrun;
            if (nr < nrun) {
                ng0 = nr * FIR_RUN;
                ng1 = ng0 + FIR_RUN < G ? ng0 + FIR_RUN : G;
                ng = ng0;
                nu = (int)((unsigned int)ng0 / (unsigned int)ntile);        // G < 2^31 (launcher)
                nt = (int)((unsigned int)ng0 - (unsigned int)nu * (unsigned int)ntile);
                more = true;
            }
        }
        return more;
    }
    __device__ __forceinline__ void advance(long long& g) { u = nu, t = nt, g = ng, g0 = ng0, g1 = ng1; }
    // A workgroup's own request has been performed before it signs off (ticket_take), so no ticket atomic can land after the reset.
    __device__ __forceinline__ void sign_off(int tid)
    {
        if (!DYN || tid != 0) return;
        (void)ticket_take<0>(pending);
        const unsigned int d = atomicAdd(counter + 1, 1u);
        if (d == gridDim.x - 1) {
            __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(counter + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

// ---- fetch and stage ----------------------------------------------------------------------------------------------------------
// Slot by slot, for tiles whose rows are not one run of bytes: slot c = tid + i * ACG_WG_FIR of `slots`, nld of them per thread;
// addr_of(c, p) -> true and the chunk's address, or false: the slot stages zeros.  NT: non-temporal loads (input read once).
template <bool NT, int MAXLD, class AddrOf>
__device__ __forceinline__ void tile_fetch_slots(int tid, int nld, int slots, uint4 (&stage)[MAXLD], AddrOf addr_of)
{
#pragma unroll
    for (int i = 0; i < MAXLD; ++i) {
        if (i < nld) {
            const int c = tid + i * ACG_WG_FIR;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (c < slots) {
                const tile_u4v* p;
                if (addr_of(c, p)) {
                    const tile_u4v x = NT ? __builtin_nontemporal_load(p) : *p;
                    v = make_uint4(x.x, x.y, x.z, x.w);
                }
            }
            stage[i] = v;
        }
    }
}
// ... and the staged slots into LDS rows `pad` bytes longer than cpr chunks
template <int MAXLD>
__device__ __forceinline__ void tile_store_slots(int tid, int nld, int slots, const uint4 (&stage)[MAXLD], unsigned char* tileL, unsigned int magic, int pad)
{
#pragma unroll
    for (int i = 0; i < MAXLD; ++i) {
        if (i < nld) {
            const int c = tid + i * ACG_WG_FIR;
            if (c < slots) {
                const int r = (int)(((unsigned int)c * magic) >> 20);
                *(uint4*)(tileL + (c << 4) + r * pad) = stage[i];
            }
        }
    }
}

// Wave-granular, for the u8 window: a tile is 64 * cpr chunks, contiguous in its stream, and a wave owns 64 consecutive chunks per
// pass, so "chunk inside the tile" is a whole-wave property (wave + 4 * i < cpr): scalar branches, no per-lane predicates, and the
// address is one uniform base per pass + a per-thread constant offset (global_load ... saddr form: no vector address arithmetic at
// all).  FULL = every tile lies completely inside the row (nwin % 64 == 0, always true for whole callbacks), which removes the
// last per-lane bound.
// The row base follows the unit (base_of(unit): its stream's first byte); it is looked up only when the unit changes (a dependent
// scalar load in front of every tile's loads would leave the workgroup without loads in flight meanwhile).
struct WaveFetch {
    const TileIds id;
    int cpr, tile_chunks, total_chunks, pad;
    unsigned int magic, voff;
    size_t tile_bytes;
    int row_unit;
    const uint8_t* __restrict__ row_base;

    __device__ __forceinline__ WaveFetch(const TileIds& id_, const FirArgs& a, const uint8_t* iq_base) : id(id_)
    {
        cpr = a.cpr;
        tile_chunks = ACG_TILE_WIN * cpr;
        total_chunks = a.nwin * cpr;
        pad = a.row_stride - a.row_bytes;
        magic = a.cpr_magic;
        voff = (unsigned int)id.tid << 4;
        tile_bytes = (size_t)tile_chunks << 4;
        row_unit = -1;
        row_base = iq_base;
    }
    template <bool NT, bool FULL, class BaseOf>
    __device__ __forceinline__ void fetch(uint4 (&stage)[FIR_MAXLD], int unit, int ft, BaseOf base_of)
    {
        if (unit != row_unit) {
            row_base = base_of(unit);
            row_unit = unit;
        }
        const uint8_t* __restrict__ tb = row_base + (size_t)ft * tile_bytes;
        const int base = ft * tile_chunks;
#pragma unroll
        for (int i = 0; i < FIR_MAXLD; ++i) {
            if (id.wave + 4 * i < cpr) {
                if (FULL || base + id.tid + i * ACG_WG_FIR < total_chunks) {
                    const tile_u4v* p = (const tile_u4v*)(tb + (size_t)i * (ACG_WG_FIR * 16) + (size_t)voff);
                    const tile_u4v x = NT ? __builtin_nontemporal_load(p) : *p;
                    stage[i] = make_uint4(x.x, x.y, x.z, x.w);
                } else {
                    stage[i] = make_uint4(0, 0, 0, 0);
                }
            }
        }
    }
    __device__ __forceinline__ void store(const uint4 (&stage)[FIR_MAXLD], unsigned char* tileL) const
    {
#pragma unroll
        for (int i = 0; i < FIR_MAXLD; ++i) {
            if (id.wave + 4 * i < cpr) {
                const int c = id.tid + i * ACG_WG_FIR;
                const int r = (int)(((unsigned int)c * magic) >> 20);
                *(uint4*)(tileL + (c << 4) + r * pad) = stage[i];
            }
        }
    }
};

// ---- samples, multiply-add, the four waves' sum, |D| -------------------------------------------------------------------------
// sample j of a chunk as (I, Q): BPS 2 the bytes as they are, unsigned (the offset is the caller's: tile_bytes_chunk, or folded
// out of the sum); 4 int16; 8 float32
template <int BPS>
__device__ __forceinline__ f2 tile_sample(const unsigned int (&qq)[4], int j)
{
    f2 x;
    if (BPS == 2) {
        const unsigned int word = qq[j >> 1];
        const unsigned int sh = (j & 1) * 16;
        x.x = (float)((word >> sh) & 0xffu);                        // rtl.c:338-339
        x.y = (float)((word >> (sh + 8)) & 0xffu);
    } else if (BPS == 4) {
        x.x = (float)(short)(qq[j] & 0xffffu);                      // soapy.c:238
        x.y = (float)((int)qq[j] >> 16);                            // soapy.c:239
    } else {
        x.x = __uint_as_float(qq[2 * j]);
        x.y = __uint_as_float(qq[2 * j + 1]);
    }
    return x;
}
// chunk c of a row as SPC = 16 / BPS samples
template <int BPS>
__device__ __forceinline__ void tile_chunk(const unsigned char* rowp, int c, f2 (&x)[16 / BPS])
{
    const uint4 q = *(const uint4*)(rowp + (c << 4));
    const unsigned int qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 16 / BPS; ++j) x[j] = tile_sample<BPS>(qq, j);
}
// the 8 samples of chunk c of a row of bytes, sample j as (j): u8 minus 127.37 (rtl.c:338-339; exact in f32), or S8: ACG_FMT_CS8's
// int8 -- xor 0x80 per word is the sample + 128 as u8, then minus 128, exactly
template <bool S8>
struct ByteChunk {
    unsigned int qq[4];
    __device__ __forceinline__ ByteChunk(const unsigned char* rowp, int c)
    {
        const uint4 q = *(const uint4*)(rowp + (c << 4));
        const unsigned int sx = S8 ? 0x80808080u : 0u;
        qq[0] = q.x ^ sx, qq[1] = q.y ^ sx, qq[2] = q.z ^ sx, qq[3] = q.w ^ sx;
    }
    __device__ __forceinline__ f2 operator()(int j) const { return tile_sample<2>(qq, j) - (S8 ? 128.0f : 127.37f); }
    __device__ __forceinline__ void all(f2 (&x)[8]) const
    {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (*this)(j);
    }
};

// SPC samples x(j) of a chunk (converted as they are asked for) times the taps tw[SPC][2] into the lane's accumulators
// (sum r*wr, sum g*wi) and (sum r*wi, sum g*wr); tile_mac: samples converted beforehand
template <int SPC, class SampleOf>
__device__ __forceinline__ void tile_mac_of(SampleOf x, const float* __restrict__ tw, f2& accA, f2& accB)
{
#pragma unroll
    for (int j = 0; j < SPC; ++j) {
        const f2 tt = x(j);
        accA = __builtin_elementwise_fma(tt, f2{tw[2 * j], tw[2 * j + 1]}, accA);
        accB = __builtin_elementwise_fma(tt, f2{tw[2 * j + 1], tw[2 * j]}, accB);
    }
}
template <int SPC>
__device__ __forceinline__ void tile_mac(const f2 (&x)[SPC], const float* __restrict__ tw, f2& accA, f2& accB)
{
    tile_mac_of<SPC>([&](int j) { return x[j]; }, tw, accA, accB);
}

__device__ __forceinline__ float4 tile_partial(f2 accA, f2 accB) { return make_float4(accA.x, accA.y, accB.x, accB.y); }

// The four waves' partial sums (sum r*wr, sum g*wi, sum r*wi, sum g*wr) of one row, wave_stride float4 apart, as (re, im): per
// component (w0 + w1) + (w2 + w3), re and im from those
__device__ __forceinline__ f2 tile_wave_sum(const float4* red, int wave_stride, int row)
{
    const float4 r0 = red[row], r1 = red[wave_stride + row], r2 = red[2 * wave_stride + row], r3 = red[3 * wave_stride + row];
    return {((r0.x + r1.x) + (r2.x + r3.x)) - ((r0.y + r1.y) + (r2.y + r3.y)), ((r0.z + r1.z) + (r2.z + r3.z)) + ((r0.w + r1.w) + (r2.w + r3.w))};
}

// window m of a channel's dm row: |D| * scale (rtl.c:353; a power of two: exact, commutes with cabsf -- 1/128 for ACG_FMT_CS8,
// 1/32768 soapy.c:241, 1/4 sdrplay.c:225), if the launch has the window
__device__ __forceinline__ void tile_store_dm(float* __restrict__ dm_row, int m, int nwin, f2 D, float scale)
{
    if (m < nwin) dm_row[m] = cabs_like_glibc(D.x, D.y) * scale;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------
// One channel per unit.  DYN = false is the persistent variant: the grid is exactly the number of workgroups the chip holds at once
// and the (channel, tile) space is cut into equal contiguous runs, one per workgroup (no partial last wave of workgroups; lab
// variants 1 and 2).  A run may cross channel boundaries; the stream/tap base pointers follow.  NT selects non-temporal loads for
// the input, which is read once.  S8: ACG_FMT_CS8 at the window lengths without a streaming kernel, and its ragged launches from
// the host feed.
template <bool NT, bool DYN, bool FULL, bool S8 = false>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_u8_persist_kernel(const FirArgs a,
                                                                     const uint8_t* __restrict__ iq_base,
                                                                     const float* __restrict__ taps_base,
                                                                     const int* __restrict__ stream_of,
                                                                     float* __restrict__ dm_base)
{
    const TileIds id;
    RunWalk<DYN> w(a.nch, a.nwin);
    if (w.none()) return;
    w.start(a.work_counter, (int*)(fir_smem + fir_persist_lds(a) - 16));
    unsigned char* tileL = fir_smem;
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);
    int c0, c1;
    tile_wave_steps(a.ntaps_pad >> 3, id.wave, c0, c1);
    WaveFetch f(id, a, iq_base);
    uint4 stage[FIR_MAXLD];
    auto row_of = [&](int ch) { return iq_base + (size_t)stream_of[ch] * a.pitch; };

    f.template fetch<NT, FULL>(stage, w.u, w.t, row_of);
    for (long long g = w.g0;;) {
        f.store(stage, tileL);
        w.request(id.tid, g);
        w.publish(id.tid, g, w.g0 + 1);
        __syncthreads();
        if (w.successor(g)) f.template fetch<NT, FULL>(stage, w.nu, w.nt, row_of);

        const float* __restrict__ taps = taps_base + (size_t)w.u * a.ntaps_pad * 2;
        f2 accA = {0.f, 0.f};
        f2 accB = {0.f, 0.f};
        const unsigned char* rowp = tileL + id.lane * a.row_stride;
        for (int c = c0; c < c1; ++c) {
            tile_mac_of<8>(ByteChunk<S8>(rowp, c), taps + (c << 4), accA, accB);
        }
        red[id.wave * 64 + id.lane] = tile_partial(accA, accB);
        __syncthreads();

        if (id.wave == 0)
            tile_store_dm(dm_base + (size_t)w.u * a.dm_pitch, w.t * ACG_TILE_WIN + id.lane, a.nwin, tile_wave_sum(red, 64, id.lane), S8 ? 1.0f / 128.0f : 1.0f);
        if (!w.more) break;
        w.advance(g);
    }
    w.sign_off(id.tid);
}

// Shared-stream variant -- rtl.c's own shape: one dongle's stream feeds several channels (up to 16,
// acarsdec.h:30).  A work unit is (group of <= FIR_KC channels of ONE stream, tile): the tile is loaded
// and converted u8 -> f32 once and every channel of the group takes its taps to the same registers.
// Per 8 complex samples: 1 ds_read_b128 + 24 conversion ops shared, 16 v_pk_fma_f32 per channel, so the
// kernel is VALU-bound at (2 + 3/K) lane-ops per channel-sample instead of HBM/fabric-bound at 5.
// The arithmetic per channel (tap split over the 4 waves, reduction order) is that of
// fir_u8_persist_kernel: both give bit-identical dm.  Partial sums meet in LDS four channels at a
// time; wave w finishes channel 4r + w.  Dynamic run dispenser as above.
// Taps come from a regrouped copy of the tap table, [group][8-sample step][channel of the group][16 floats]
// (regroup_taps_kernel), so that one scalar base + immediate offsets reaches all channels of a step.
// S8: ACG_FMT_CS8 with several channels per stream where the matrix kernel does not take the launch (or ACG_FIR_MM=0).
template <bool FULL, bool S8 = false>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_u8_shared_kernel(const FirArgs a,
                                                                    const uint8_t* __restrict__ iq_base,
                                                                    const float* __restrict__ taps_base,
                                                                    const int4* __restrict__ groups,
                                                                    const int* __restrict__ group_ch,
                                                                    float* __restrict__ dm_base)
{
    const TileIds id;
    RunWalk<true> w(a.ngroups, a.nwin);
    if (w.none()) return;
    w.start(a.work_counter, (int*)(fir_smem + fir_shared_lds(a) - 16));
    unsigned char* tileL = fir_smem;
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);      // [4 channels][4 waves][64]
    int c0, c1;
    tile_wave_steps(a.ntaps_pad >> 3, id.wave, c0, c1);
    WaveFetch f(id, a, iq_base);
    uint4 stage[FIR_MAXLD];
    auto row_of = [&](int grp) { return iq_base + (size_t)groups[grp].x * a.pitch; };

    f.template fetch<true, FULL>(stage, w.u, w.t, row_of);
    for (long long g = w.g0;;) {
        f.store(stage, tileL);
        w.request(id.tid, g);
        w.publish(id.tid, g, w.g0 + 1);
        __syncthreads();
        if (w.successor(g)) f.template fetch<true, FULL>(stage, w.nu, w.nt, row_of);

        const int4 gi = groups[w.u];                                        // wave-uniform
        const int kc = gi.z;
        const float* __restrict__ gt = taps_base + (size_t)gi.y * a.ntaps_pad * 2;
        f2 accA[FIR_KC], accB[FIR_KC];
#pragma unroll
        for (int k = 0; k < FIR_KC; ++k) {
            accA[k] = {0.f, 0.f};
            accB[k] = {0.f, 0.f};
        }
        const unsigned char* rowp = tileL + id.lane * a.row_stride;
        auto taps_pass = [&](auto full) {
            constexpr bool ALLK = decltype(full)::value;
            const int kcc = ALLK ? FIR_KC : kc;
            for (int c = c0; c < c1; ++c) {
                const float* __restrict__ wc = gt + (size_t)(c * kcc) * 16;
                f2 x[8];
                ByteChunk<S8>(rowp, c).all(x);
#pragma unroll
                for (int k = 0; k < FIR_KC; ++k)
                    if (ALLK || k < kc) tile_mac(x, wc + k * 16, accA[k], accB[k]);
            }
        };
        if (kc == FIR_KC) taps_pass(std::true_type{});
        else taps_pass(std::false_type{});

        const int m = w.t * ACG_TILE_WIN + id.lane;
#pragma unroll
        for (int r = 0; r < FIR_KC / 4; ++r) {
            if (4 * r < kc) {                                               // uniform
                if (r > 0) __syncthreads();                                 // round r-1's reads are done
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) red[(kk * 4 + id.wave) * 64 + id.lane] = tile_partial(accA[4 * r + kk], accB[4 * r + kk]);
                __syncthreads();
                if (4 * r + id.wave < kc) {
                    const int mych = group_ch[gi.y + 4 * r + id.wave];      // wave-uniform
                    tile_store_dm(dm_base + (size_t)mych * a.dm_pitch, m, a.nwin, tile_wave_sum(red + (id.wave * 4) * 64, 64, id.lane), S8 ? 1.0f / 128.0f : 1.0f);
                }
            }
        }
        if (!w.more) break;
        w.advance(g);
    }
    w.sign_off(id.tid);
}

// The other front ends' sample formats: same tile scheme, 4 bytes per input sample (FMT_CF32: 8).  A row (one window) is 4*M bytes
// in LDS (FMT_CF32: 8*M); for FMT_SPLIT it is [I half | Q half]; windows longer than 52 chunks (Airspy: 480 / 800 samples) pass
// through LDS in K column slices of cpr chunks, and the partial sums stay in registers across the slices of one tile.  Static
// contiguous partition of the (channel, tile) space, non-temporal loads, taps through scalar loads.
template <int FMT>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_fmt_kernel(const FirArgs a,
                                                              const uint8_t* __restrict__ in_base,
                                                              const float* __restrict__ taps_base,
                                                              const int* __restrict__ stream_of,
                                                              float* __restrict__ dm_base)
{
    SliceWalk w(a.nch, a.nwin, ACG_TILE_WIN, a.kseg);
    if (w.u1 <= 0) return;
    const int cpr = a.cpr;                              // 16-byte chunks per LDS row (one slice)
    const int half = cpr >> 1;                          // FMT_SPLIT: chunks per plane row (one slice)
    const int tile_chunks = ACG_TILE_WIN * cpr;
    const int pad = a.row_stride - (cpr << 4);
    unsigned char* tileL = fir_smem;
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);
    constexpr int SPC = (FMT == FMT_SPLIT) ? 8 : (FMT == FMT_CF32) ? 2 : 4;     // samples (taps) per inner step
    const int nstep_total = a.ntaps_pad / SPC;
    const int nld = (tile_chunks + ACG_WG_FIR - 1) / ACG_WG_FIR;
    uint4 stage[FMT_MAXLD];

    auto fetch = [&](int fch, int ft, int fk) {
        const uint8_t* __restrict__ src = in_base + (size_t)stream_of[fch] * a.pitch;
        const int col0 = fk * cpr;
        tile_fetch_slots<true>(w.tid, nld, tile_chunks, stage, [&](int c, const tile_u4v*& p) {
            int r, col;
            tile_slot(c, a.cpr_magic, cpr, r, col);
            const int win = ft * ACG_TILE_WIN + r;
            if (!(win < a.nwin && col0 + col < a.cpr_total)) return false;
            size_t off;
            if (FMT == FMT_SPLIT)           // I plane, then Q plane a.plane bytes further
                off = (col < half) ? (size_t)win * (a.row_bytes >> 1) + ((size_t)col << 4)
                                   : a.plane + (size_t)win * (a.row_bytes >> 1) + ((size_t)(col - half) << 4);
            else
                off = (size_t)win * a.row_bytes + ((size_t)(col0 + col) << 4);
            p = (const tile_u4v*)(src + off);
            return true;
        });
    };

    f2 accA = {0.f, 0.f};       // CS16/SPLIT/CF32: (sum r*wr, sum g*wi)   F32R: (sum s*wr, sum s*wi)
    f2 accB = {0.f, 0.f};       // CS16/SPLIT/CF32: (sum r*wi, sum g*wr)
    fetch(w.ch, w.t, 0);
    for (long long u = 0; u < w.u1; ++u) {
        tile_store_slots(w.tid, nld, tile_chunks, stage, tileL, a.cpr_magic, pad);
        __syncthreads();
        const bool last = w.successor(true);            // last slice of this tile
        if (u + 1 < w.u1) fetch(w.nch, w.nt, w.nk);

        // this slice's inner steps, split over the 4 waves
        int c0, c1;
        tile_wave_steps((FMT == FMT_SPLIT) ? nstep_total : max(0, min(cpr, nstep_total - w.k * cpr)), w.wave, c0, c1);
        const float* __restrict__ taps = taps_base + (size_t)w.ch * a.ntaps_pad * 2 + (size_t)w.k * cpr * SPC * 2;
        const unsigned char* rowp = tileL + w.lane * a.row_stride;
        for (int c = c0; c < c1; ++c) {
            const float* __restrict__ tw = taps + c * SPC * 2;                 // wave-uniform
            if constexpr (FMT == FMT_SPLIT) {
                f2 xi[4], xq[4], x[8];
                tile_chunk<4>(rowp, c, xi);                                    // int16 halves of a word: (even, odd) samples of a plane
                tile_chunk<4>(rowp, c + half, xq);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = (j & 1) ? f2{xi[j >> 1].y, xq[j >> 1].y} : f2{xi[j >> 1].x, xq[j >> 1].x};   // sdrplay.c:219-220
                tile_mac(x, tw, accA, accB);
            } else if constexpr (FMT == FMT_F32R) {
                const float4 q = *(const float4*)(rowp + (c << 4));
                const float sv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) accA = __builtin_elementwise_fma(f2{sv[j], sv[j]}, f2{tw[2 * j], tw[2 * j + 1]}, accA);   // air.c:315-316: wf[i] * S
            } else {
                f2 x[SPC];
                tile_chunk<FMT == FMT_CF32 ? 8 : 4>(rowp, c, x);               // soapy.c:238-239 (float32: without the conversion)
                tile_mac(x, tw, accA, accB);
            }
        }
        if (last) {                                     // reduce the 4 waves, emit |D|
            red[w.wave * 64 + w.lane] = tile_partial(accA, accB);
            accA = {0.f, 0.f};
            accB = {0.f, 0.f};
            __syncthreads();
            if (w.wave == 0) {
                f2 D;
                if (FMT == FMT_F32R) {                  // real samples: re and im are .x and .y alone
                    const float4 r0 = red[w.lane], r1 = red[64 + w.lane], r2 = red[128 + w.lane], r3 = red[192 + w.lane];
                    D = {(r0.x + r1.x) + (r2.x + r3.x), (r0.y + r1.y) + (r2.y + r3.y)};
                } else {
                    D = tile_wave_sum(red, 64, w.lane);
                }
                tile_store_dm(dm_base + (size_t)w.ch * a.dm_pitch, w.t * ACG_TILE_WIN + w.lane, a.nwin, D, a.out_scale);
            }
        } else {
            __syncthreads();                            // the slice in LDS is overwritten next round
        }
        w.advance();
    }
}

// ---- launching them -----------------------------------------------------------------------------------------------------------
// the whole / ragged pair of a u8 tile kernel: FULL where every tile of the launch is complete (whole callbacks)
template <class... P, class... A>
static int launch_whole_or_ragged(void (*whole)(P...), void (*ragged)(P...), int nwin, long long grid, size_t lds, hipStream_t stream, A... args)
{
    void (*kernel)(P...) = nwin % ACG_TILE_WIN == 0 ? whole : ragged;
    FIR_LAUNCH(kernel, dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, stream, args...);
    return (int)hipGetLastError();
}

// fir_u8_persist_kernel with the run dispenser: acg_launch_fir's fallback, and the signed twin's launch in fir_iq.hip
template <bool S8>
static int launch_persist(const FirArgs& b, const FirArgs* a, int num_cu, hipStream_t stream)
{
    const size_t lds = fir_persist_lds(*a);
    const long long G = acg_fir_tile_units(a->nch, a->nwin, ACG_TILE_WIN);
    if (G >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const long long grid = acg_fir_tile_grid(a->ncu > 0 ? a->ncu : num_cu, lds, 5, a->wg_per_cu, true, G, FIR_RUN);
    return launch_whole_or_ragged(fir_u8_persist_kernel<true, true, true, S8>, fir_u8_persist_kernel<true, true, false, S8>, a->nwin, grid, lds, stream,
                                  b, a->iq, a->taps, a->stream_of, a->dm);
}

// fir_fmt_kernel: acg_launch_fir_fmt's and acg_launch_fir_cf32's second step, four workgroups per CU at most
template <int FMT>
static int launch_fmt(const FirArgs* a, int num_cu, hipStream_t stream)
{
    const size_t lds = fir_fmt_lds(*a);
    if (lds > 64 * 1024) return (int)hipErrorInvalidValue;
    const long long grid = acg_fir_tile_grid(a->ncu > 0 ? a->ncu : num_cu, lds, 4, 0, false, acg_fir_tile_units(a->nch, a->nwin, ACG_TILE_WIN));
    FIR_LAUNCH(fir_fmt_kernel<FMT>, dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, stream, *a, a->iq, a->taps, a->stream_of, a->dm);
    return (int)hipGetLastError();
}

#endif /* ACG_FIR_TILE_KERNEL_H */
