// fir_grid_kernel.h -- what the kernels of fir_rate.hip and fir_long.hip are both made of, on top of the tile family's common parts
// (fir_tile_kernel.h; the siblings of its fir_fmt_kernel): a tile of ACG_TILE_WIN windows goes through LDS one padded row per
// window, lane = window, the four waves split the taps, partial sums meet in LDS, windows longer than a slice go through in column
// slices; a workgroup walks a static contiguous share of the (channel, tile) space and fetches unit u + 1 into registers while
// it computes unit u.  The ids, the static share, the slot decode, the wave split, the sample conversions, the multiply-add, the
// four waves' sum and the launchers' grid are the family's.  What the grid adds is that a row -- a window -- begins at any sample of its stream:
//   * the rows are fetched in ALIGNED 16-byte non-temporal chunks, per row from its start rounded down to 16 bytes, so a chunk
//     that two windows share is fetched for both (it hits L2 the second time): one aligned chunk more per row than the window has
//     (grid_fetch; fir_grid.h's plan counts it);
//   * and RE-ALIGNED ON THE WAY INTO LDS: a chunk is stored at its place minus the row's skew, in 8- or 4-byte pieces (the skew
//     is a multiple of the sample size: 2, 4 or 8 bytes).  A row has 16 bytes in front and behind its data, so the first and the
//     last chunk need no predicate (grid_stage_store);
//   * 2-byte samples are stored minus the skew's whole words, and a lane whose row lies one half word late shifts its 16 bytes
//     into place with v_alignbit (grid_read_chunk): stored in 2-byte pieces, the compiler makes one ds_write_b128 at 2-byte
//     alignment of them, which the hardware performs piece by piece -- profiles/LEDGER.md.
// Every row then begins at its own window's start: the reads are the sibling's aligned ds_read_b128 at an odd row stride, and the
// taps are wave-uniform scalar loads.  Where a row begins is the kernel's own rule, handed to grid_fetch and grid_stage_store as
// a functor; so are its windows, accumulators and outputs.
#pragma once
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "fir_grid.h"
#include "fir_tile_kernel.h"

// one row of a tile, as grid_fetch is told of it
struct GridRow {
    const uint8_t* src;             // the row's stream (or its history)
    unsigned long long base, lim;   // bytes from src: the row's first sample rounded down to 16; what may be read
    int skew;                       // the first sample's bytes behind base, 0 .. 15
    bool exists;                    // a window of the launch (and of the context)
};

// A workgroup's share of the launch (the family's static share) and its walk over it: units (channel ch, tile t, slice k), slices
// innermost.  The walk is SliceWalk's, spelled out: derived from it, fir_long_kernel compiles to other text and its shared-stream
// arm runs 0.3 % slower, outside the parent's spread (profiles/LEDGER.md, "Tile down-converters on one skeleton").
struct GridWalk : TileIds {
    const FirGridArgs& a;
    int ntile;
    int cprl, slots, nld;           // aligned chunks loaded per row and slice (one more than it holds), load slots of a slice, per thread
    int win_bytes;
    long long u1;                   // the units of this workgroup
    int ch, t, k;                   // the unit in LDS
    int nch, nt, nk;                // its successor, the unit being fetched

    // tile_out: outputs per tile; bps: the instantiation's bytes per sample
    __device__ __forceinline__ GridWalk(const FirGridArgs& a_, int tile_out, int bps) : a(a_)
    {
        ntile = (a.nwin + tile_out - 1) / tile_out;
        long long g0, g1;
        tile_static_share((long long)a.nch * ntile, g0, g1);
        cprl = a.cpr + 1;
        slots = ACG_TILE_WIN * cprl;
        nld = (slots + ACG_WG_FIR - 1) / ACG_WG_FIR;
        win_bytes = a.decim * bps;
        u1 = (g1 - g0) * a.kseg;                        // none: the loop does not run
        ch = (int)(g0 / ntile);
        t = (int)(g0 - (long long)ch * ntile);
        k = 0;
    }
    // load slot c of a slice -> its row and its aligned chunk in the row's slice
    __device__ __forceinline__ void slot(int c, int& r, int& col) const { tile_slot(c, a.ld_magic, cprl, r, col); }
    // the successor of the unit in LDS (round -1, !live: the first unit itself); true: it begins another tile
    __device__ __forceinline__ bool successor(bool live)
    {
        nch = ch, nt = t, nk = live ? k + 1 : 0;
        if (!live || nk != a.kseg) return false;
        nk = 0;
        if (++nt == ntile) { nt = 0; ++nch; }
        return true;
    }
    __device__ __forceinline__ void advance() { ch = nch, t = nt, k = nk; }
    // this slice's chunks, split over the 4 waves
    __device__ __forceinline__ void wave_chunks(int& c0, int& c1) const { tile_wave_steps(max(0, min(a.cpr, a.cpr_total - k * a.cpr)), wave, c0, c1); }
};

// The loads of slice w.nk of the successor's tile into the staging registers; row_of(r) -> GridRow.  A slot is loaded if its row
// exists and the chunk holds samples of the window and lies inside what may be read; the others stage zeros.
// (In its own words, not through the family's tile_fetch_slots: with the predicate behind a functor the compiler spills 20 fewer
// SGPRs and the kernels run 1-3 % slower -- rate-cu8 1.077 -> 1.110 ms, the filter at J = 4 cs16 2.66 -> 2.74 ms; profiles/LEDGER.md,
// "Tile down-converters on one skeleton".)
template <int MAXLD, class RowOf>
__device__ __forceinline__ void grid_fetch(const GridWalk& w, uint4 (&stage)[MAXLD], RowOf row_of)
{
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int i = 0; i < MAXLD; ++i) {
        if (i < w.nld) {
            const int c = w.tid + i * ACG_WG_FIR;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (c < w.slots) {
                int r, col;
                w.slot(c, r, col);
                const GridRow row = row_of(r);
                const int colg = w.nk * w.a.cpr + col;                    // aligned chunk of the row
                const unsigned long long off = row.base + ((unsigned long long)colg << 4);
                if (row.exists && (colg << 4) < row.skew + w.win_bytes && off + 16 <= row.lim) {
                    const u4v x = __builtin_nontemporal_load((const u4v*)(row.src + off));
                    v = make_uint4(x.x, x.y, x.z, x.w);
                }
            }
            stage[i] = v;
        }
    }
}

// The staged slice into LDS, realigned: a chunk's place in its row minus the row's skew, behind the 16 bytes in front (2-byte
// samples: minus the skew's whole words only -- an odd half word is the reader's, grid_read_chunk); skew_of(r): of the tile in LDS.
template <int BPS, int MAXLD, class SkewOf>
__device__ __forceinline__ void grid_stage_store(const GridWalk& w, const uint4 (&stage)[MAXLD], unsigned char* tileL, SkewOf skew_of)
{
#pragma unroll
    for (int i = 0; i < MAXLD; ++i) {
        if (i < w.nld) {
            const int c = w.tid + i * ACG_WG_FIR;
            if (c < w.slots) {
                int r, col;
                w.slot(c, r, col);
                unsigned char* dst = tileL + r * w.a.row_stride + 16 + (col << 4) - (skew_of(r) & (BPS == 2 ? 12 : 15));
                if (BPS == 8) {
                    ((uint2*)dst)[0] = make_uint2(stage[i].x, stage[i].y);
                    ((uint2*)dst)[1] = make_uint2(stage[i].z, stage[i].w);
                } else {
                    ((unsigned int*)dst)[0] = stage[i].x; ((unsigned int*)dst)[1] = stage[i].y;
                    ((unsigned int*)dst)[2] = stage[i].z; ((unsigned int*)dst)[3] = stage[i].w;
                }
            }
        }
    }
}

// Chunk c of the lane's row (rowp: behind the 16 bytes in front).  2-byte samples: a row whose skew is an odd number of half words
// lies one half word late (its words were stored whole); the lane shifts its 16 bytes into place with the next word, v_alignbit
// by 0 or 16
template <int BPS>
__device__ __forceinline__ void grid_read_chunk(const unsigned char* rowp, int c, int skew, unsigned int (&qq)[4])
{
    const uint4 q = *(const uint4*)(rowp + (c << 4));
    qq[0] = q.x; qq[1] = q.y; qq[2] = q.z; qq[3] = q.w;
    if (BPS == 2) {
        const unsigned int nx = *(const unsigned int*)(rowp + (c << 4) + 16), half = (unsigned int)(skew & 2) * 8u;
        qq[0] = __builtin_amdgcn_alignbit(q.y, q.x, half);
        qq[1] = __builtin_amdgcn_alignbit(q.z, q.y, half);
        qq[2] = __builtin_amdgcn_alignbit(q.w, q.z, half);
        qq[3] = __builtin_amdgcn_alignbit(nx, q.w, half);
    }
}

// the family's sample conversion, multiply-add and four-wave sum under the names the grid kernels call them by
template <int BPS>
__device__ __forceinline__ f2 grid_sample(const unsigned int (&qq)[4], int j) { return tile_sample<BPS>(qq, j); }
template <int SPC>
__device__ __forceinline__ void grid_mac(const f2 (&x)[SPC], const float* __restrict__ tw, f2& accA, f2& accB) { tile_mac(x, tw, accA, accB); }
__device__ __forceinline__ f2 grid_wave_sum(const float4* red, int wave_stride, int row) { return tile_wave_sum(red, wave_stride, row); }

// The launchers' grid: as many workgroups as stay resident (per_cu_max of them on a CU, or fewer by their LDS), at most one per
// (channel, tile).
static inline int grid_resident_blocks(const FirGridArgs* a, size_t lds, int per_cu_max, int tile_out, long long* grid)
{
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    *grid = acg_fir_tile_grid(a->ncu > 0 ? a->ncu : num_cu, lds, per_cu_max, 0, false, acg_fir_tile_units(a->nch, a->nwin, tile_out));
    return 0;
}
