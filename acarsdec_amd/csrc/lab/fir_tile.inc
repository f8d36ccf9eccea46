// csrc/lab/fir_tile.inc -- round 1's first kernel (ACG_FIR_VARIANT=0): LAB BUILD ONLY (libacarsdec_amd_lab.so, -DACG_LAB).  Textually included by fir.hip, which
// provides the helpers it uses; the product library never sees this file (tests/test_host_logic.py compares the product's
// kernel list; the product object is byte-identical with and without it).
__global__ __launch_bounds__(ACG_WG_FIR) void fir_u8_tile_kernel(const FirArgs a,
                                                                  const uint8_t* __restrict__ iq_base,
                                                                  const float* __restrict__ taps_base,
                                                                  const int* __restrict__ stream_of,
                                                                  float* __restrict__ dm_base)
{
    const TileIds id;
    const int lane = id.lane, wave = id.wave;
    const int ch = blockIdx.x / a.nseg;
    const int seg = blockIdx.x - ch * a.nseg;
    const int ntile = (a.nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const int t0 = (int)((long long)ntile * seg / a.nseg);
    const int t1 = (int)((long long)ntile * (seg + 1) / a.nseg);
    if (t0 >= t1) return;

    const uint8_t* __restrict__ src = iq_base + (size_t)stream_of[ch] * a.pitch;
    const float* __restrict__ taps = taps_base + (size_t)ch * a.ntaps_pad * 2;

    const int tile_chunks = ACG_TILE_WIN * a.cpr;
    const int total_chunks = a.nwin * a.cpr;            // valid 16-byte chunks of this stream row
    unsigned char* tileL = fir_smem;
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);
    int c0, c1;
    tile_wave_steps(a.ntaps_pad >> 3, wave, c0, c1);     // chunks that carry taps
    const int nld = (tile_chunks + ACG_WG_FIR - 1) / ACG_WG_FIR;
    uint4 stage[FIR_MAXLD];
    auto fetch = [&](int t) {
        const int base = t * tile_chunks;
        tile_fetch_slots<false>(id.tid, nld, tile_chunks, stage, [&](int c, const tile_u4v*& p) {
            p = (const tile_u4v*)(src + ((size_t)(base + c) << 4));
            return base + c < total_chunks;
        });
    };

    fetch(t0);
    for (int t = t0; t < t1; ++t) {
        tile_store_slots(id.tid, nld, tile_chunks, stage, tileL, a.cpr_magic, a.row_stride - a.row_bytes);     // registers -> LDS (padded rows)
        __syncthreads();
        if (t + 1 < t1) fetch(t + 1);                   // the next tile's loads stay in flight during the compute below

        // ---- this wave's share of the taps, lane = window
        f2 accA = {0.f, 0.f};       // (sum tr*wr, sum ti*wi)
        f2 accB = {0.f, 0.f};       // (sum tr*wi, sum ti*wr)
        const unsigned char* rowp = tileL + lane * a.row_stride;
        for (int c = c0; c < c1; ++c) {
            tile_mac_of<8>(ByteChunk<false>(rowp, c), taps + (c << 4), accA, accB);    // wave-uniform -> scalar loads
        }
        red[wave * 64 + lane] = tile_partial(accA, accB);
        __syncthreads();

        if (wave == 0) tile_store_dm(dm_base + (size_t)ch * a.dm_pitch, t * ACG_TILE_WIN + lane, a.nwin, tile_wave_sum(red, 64, lane), 1.0f);
        // the barrier at the top of the next iteration orders wave 0's reads of `red`
        // before anyone rewrites it.
    }
}

