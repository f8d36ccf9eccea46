// csrc/lab/fir_dma.inc -- the LDS-DMA variant (ACG_FIR_VARIANT=4): LAB BUILD ONLY (libacarsdec_amd_lab.so, -DACG_LAB).  Textually included by fir.hip, which
// provides the helpers it uses; the product library never sees this file (tests/test_host_logic.py compares the product's
// kernel list; the product object is byte-identical with and without it).
// LDS-DMA variant (rows that are an odd number of 16-byte slots, e.g. M = 200: no padding needed, so the
// LDS image of a tile is the linear image of its bytes in HBM).  `global_load_lds_dwordx4 ... nt` moves
// 1 KiB per wave-instruction straight into LDS: no staging VGPRs, no ds_write pass, one barrier per
// tile.  Two tile buffers: the DMA of tile t+1 lands while tile t is computed.  The run walk of
// the register-staged kernel (RunWalk).  LDS: 2 tiles + 2 reduction buffers -> 2 workgroups per CU.
__global__ __launch_bounds__(ACG_WG_FIR) void fir_u8_dma_kernel(const FirArgs a,
                                                                 const uint8_t* __restrict__ iq_base,
                                                                 const float* __restrict__ taps_base,
                                                                 const int* __restrict__ stream_of,
                                                                 float* __restrict__ dm_base)
{
    const TileIds id;
    const int lane = id.lane, wave = id.wave;
    const int cpr = a.cpr;                               // odd
    const int tile_bytes = ACG_TILE_WIN * a.row_bytes;   // = cpr KiB
    const int total_chunks = a.nwin * cpr;
    unsigned char* buf0 = fir_smem;
    float4* red = (float4*)(fir_smem + 2 * tile_bytes);  // [2][4][64]
    RunWalk<true> w(a.nch, a.nwin);
    if (w.none()) return;
    w.start(a.work_counter, (int*)(fir_smem + 2 * tile_bytes + 2 * 4 * 64 * sizeof(float4)));
    int c0, c1;
    tile_wave_steps(a.ntaps_pad >> 3, wave, c0, c1);

    auto issue = [&](int fch, int ft, int b) {
        const uint8_t* __restrict__ src = iq_base + (size_t)stream_of[fch] * a.pitch;
        const int base = ft * ACG_TILE_WIN * cpr;
        unsigned char* dst = buf0 + b * tile_bytes;
        for (int q = wave; q < cpr; q += 4) {            // wave-uniform: 1 KiB per instruction
            int c = base + q * 64 + lane;
            if (c >= total_chunks) c = total_chunks - 1;  // partial last tile: rows nobody stores
            // inline asm: as a builtin the compiler orders every later ds_read behind it with vmcnt(0)
            const unsigned char* gp = src + ((size_t)c << 4);
            const unsigned int ldst = __builtin_amdgcn_readfirstlane((unsigned int)(uintptr_t)(dst + q * 1024));
            unsigned int keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(gp), "s"(ldst) : "memory");
        }
    };

    issue(w.u, w.t, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (long long g = w.g0;;) {
        w.request(id.tid, g);
        if (w.successor(g)) issue(w.nu, w.nt, cur ^ 1);

        const float* __restrict__ taps = taps_base + (size_t)w.u * a.ntaps_pad * 2;
        f2 accA = {0.f, 0.f};
        f2 accB = {0.f, 0.f};
        const unsigned char* rowp = buf0 + cur * tile_bytes + lane * a.row_bytes;
        for (int c = c0; c < c1; ++c) {
            tile_mac_of<8>(ByteChunk<false>(rowp, c), taps + (c << 4), accA, accB);
        }
        float4* rd = red + cur * 256;
        rd[wave * 64 + lane] = tile_partial(accA, accB);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of the next tile has landed
        w.publish(id.tid, g, w.g0);                            // on the run's first tile, published by the barrier below
        __syncthreads();

        if (wave == 0) tile_store_dm(dm_base + (size_t)w.u * a.dm_pitch, w.t * ACG_TILE_WIN + lane, a.nwin, tile_wave_sum(rd, 64, lane), 1.0f);
        if (!w.more) break;
        w.advance(g);
        cur ^= 1;
    }
    w.sign_off(id.tid);
}

