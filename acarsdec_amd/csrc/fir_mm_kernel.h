// fir_mm_kernel.h -- the text of fir_mm.hip's shared-stream kernel, included once per sample type: FIR_MM_KERNEL names the
// kernel, FIR_MM_S8 says whether the bytes are u8 I/Q (0: rtl.c's, xor 0x80 and the channel's constant) or int8 I/Q (1:
// ACG_FMT_CS8 -- the bytes ARE the int8 operands: no xor, no constant (MmChan's dc is the u8 offset's and is not read), the same
// digits, the same exact int32 sums, the same single rounding; |D| / 128).  Two copies of one text, not a template parameter:
// the u8 kernel keeps its name and compiles to what it compiled to before the second sample type existed.
template <int CPR, int STAGES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(STAGES == 1 ? 2 : 1, STAGES == 1 ? 2 : 1)))
void FIR_MM_KERNEL(const FirArgs a, const uint8_t* __restrict__ iq_base, const u4m_t* __restrict__ img,
                   const MmChan* __restrict__ mmch, const int4* __restrict__ groups, const int* __restrict__ group_ch,
                   float* __restrict__ dm_base)
{
    constexpr bool S8 = FIR_MM_S8 != 0;
    typedef FirMM<CPR> F;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char* tile = mm_smem + wave * F::WAVE_LDS;
    MmChan* constL = (MmChan*)(tile + F::TILE_LDS);
    const unsigned int wpg = blockDim.x >> 6;
    const unsigned int nwaves = gridDim.x * wpg;
    const unsigned int wg = blockIdx.x * wpg + (unsigned int)wave;
    const unsigned int tpr = (unsigned int)a.run_pairs;                              // tiles per run (launcher)
    const unsigned int rpg = ((unsigned int)a.nwin / F::WIN) / tpr;                  // runs per group
    const unsigned int nrun = (unsigned int)a.ngroups * rpg;
    unsigned int* ctr = a.work_counter;
    const int w = lane & 31, h = lane >> 5;
    const unsigned char* rowp = tile + w * F::S + 16 * h;

    // where this lane's chunk of wave-load q goes in the LDS tile, and whether the chunk exists (the last load of an odd tile)
    unsigned int voff[F::NLD];
    unsigned int ldsoff[F::NLD];
#pragma unroll
    for (int q = 0; q < F::NLD; ++q) {
        const unsigned int c = (unsigned int)(q * 64 + lane);
        const unsigned int r = (c * ((65536u + CPR - 1) / CPR)) >> 16;                // c / CPR for c < 2048
        ldsoff[q] = (c << 4) + r * (unsigned int)(F::S - F::RB);
        voff[q] = c < (unsigned int)(F::WIN * CPR) ? ((unsigned int)lane << 4) : 0x80000000u;   // past the descriptor: returns 0, touches nothing
    }

    unsigned int run = wg;
    if (run >= nrun) {
        unsigned int t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run = nwaves + (unsigned int)__builtin_amdgcn_readfirstlane((int)t);
    }
    while (run < nrun) {
        const unsigned int g = run / rpg;
        const unsigned int t0 = (run - g * rpg) * tpr;
        const int4 gi = groups[g];
        const int kc = gi.z;
        const uint8_t* base = iq_base + (size_t)gi.x * a.pitch + (size_t)t0 * F::TILE_BYTES;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)(tpr * (unsigned int)F::TILE_BYTES), 0x00020000);
        u4m_t stA[F::NLD], stB[F::NLD];
#pragma unroll
        for (int q = 0; q < F::NLD; ++q) stA[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff[q], q * 1024, 2 /* nt */);
        if (STAGES == 2 && tpr > 1) {
#pragma unroll
            for (int q = 0; q < F::NLD; ++q) stB[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff[q], F::TILE_BYTES + q * 1024, 2);
        }

        // the group's A operand (digits of its <= 8 tap tables) into registers, its channels' constants into LDS
        v4i_t tap[F::KS][2];
        {
            const v4i_t* ip = (const v4i_t*)img + (size_t)g * F::IMG_V4 + lane;
#pragma unroll
            for (int k = 0; k < F::KS; ++k) {
                tap[k][0] = ip[(k * 2 + 0) * 64];
                tap[k][1] = ip[(k * 2 + 1) * 64];
            }
            if (lane < 8) {
                const double4* src = (const double4*)(mmch + group_ch[gi.y + (lane < kc ? lane : 0)]);
                double4 v = *src;
                if (lane >= kc) v = make_double4(0.0, 0.0, 0.0, 0.0);
                *(double4*)(constL + lane) = v;
            }
        }
        // the four channels this lane finishes: local index 4 m + (lane >> 5) + 2 chhi
        float* dmrow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int chl = 4 * (i >> 1) + h + 2 * (i & 1);
            const int ch = chl < kc ? group_ch[gi.y + chl] : -1;
            dmrow[i] = ch >= 0 ? dm_base + (size_t)ch * a.dm_pitch + (size_t)t0 * F::WIN + w : nullptr;
        }

        auto tile_step = [&](u4m_t (&st)[F::NLD], unsigned int t) {
            // ---- tile t: registers -> LDS (the previous tile's reads are older LDS operations of this wave: they are done)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < F::NLD; ++q)
                if (q + 1 < F::NLD || (F::WIN * CPR) % 64 == 0 || lane < (F::WIN * CPR) % 64) *(u4m_t*)(tile + ldsoff[q]) = st[q];
            // ---- ask for tile t + STAGES (lands in these registers while this one and the next are multiplied)
            if (t + STAGES < tpr) {
#pragma unroll
                for (int q = 0; q < F::NLD; ++q)
                    st[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff[q], (int)((t + STAGES) * (unsigned int)F::TILE_BYTES) + q * 1024, 2);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // ---- KS k-steps, two MFMAs each (channels 0-3 / 4-7 of the group)
            v16i_t acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            v16i_t acc1 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < F::KS; ++k) {
                u4m_t d = *(const u4m_t*)(rowp + 32 * k);
                if (!S8) d ^= 0x80808080u;                                             // u8 -> u8 - 128 as int8
                v4i_t b;
                b[0] = (int)d[0]; b[1] = (int)d[1]; b[2] = (int)d[2]; b[3] = (int)d[3];
                acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(tap[k][0], b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(tap[k][1], b, acc1, 0, 0, 0);
            }
            // ---- lane = (window, channel parity): four channels x (re, im) x four digits, all in this lane
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int chl = 4 * (i >> 1) + h + 2 * (i & 1);
                const MmChan cc = constL[chl];
                float v[2];
#pragma unroll
                for (int ri = 0; ri < 2; ++ri) {
                    const int r0 = 4 * (2 * (i & 1) + ri);                            // register group reg >> 2 = re/im + 2 chhi
                    const int a0 = (i >> 1) ? acc1[r0 + 0] : acc0[r0 + 0];
                    const int a1 = (i >> 1) ? acc1[r0 + 1] : acc0[r0 + 1];
                    const int a2 = (i >> 1) ? acc1[r0 + 2] : acc0[r0 + 2];
                    const int a3 = (i >> 1) ? acc1[r0 + 3] : acc0[r0 + 3];
                    const int lo = a1 * 256 + a0;                                      // |a1| < 2^23 - 2^15: fits
                    const int hi = a3 * 256 + a2;                                      // |a3| <= 400 * 128 * 65
                    const double D = __fma_rn((double)hi, 65536.0, (double)lo);        // exact (47 bits)
                    v[ri] = S8 ? (float)(D * cc.scale)                                 // (a power of two: the product is exact)
                               : (float)__fma_rn(D, cc.scale, ri ? cc.dc_im : cc.dc_re);   // the one rounding of the sum
                }
                if (dmrow[i]) {
                    dmrow[i][0] = S8 ? mm_cabs(v[0], v[1]) * (1.0f / 128.0f) : mm_cabs(v[0], v[1]);
                    dmrow[i] += F::WIN;
                }
            }
        };
        if (STAGES == 1) {
            for (unsigned int t = 0; t < tpr; ++t) tile_step(stA, t);
        } else {
            for (unsigned int t = 0; t < tpr; t += 2) {
                tile_step(stA, t);
                if (t + 1 < tpr) tile_step(stB, t + 1);
            }
        }
        unsigned int tk = 0;
        if (lane == 0) tk = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run = nwaves + (unsigned int)__builtin_amdgcn_readfirstlane((int)tk);
    }
    if (lane == 0) {
        const unsigned int d = atomicAdd(ctr + 1, 1u);
        if (d == nwaves - 1) {                                      // every wave's draws have been answered: re-arm
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

