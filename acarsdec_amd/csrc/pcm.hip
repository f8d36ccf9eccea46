// pcm.hip -- the 12.5 kHz front ends' input (soundfile.c:65-77, alsa.c:114-122): interleaved PCM frames [nframes][nch], int16 or
// float32, become columns [0, nframes) of the planar dm rows the demodulator reads.  S16 is sf_read_float's normalisation of a
// PCM16 file, (float)x * 2^-15: exact in f32 (a 16-bit integer times a power of two), so no rounding mode or contraction can
// show.  F32 is moved as a 32-bit word: no float instruction touches it (NaN payloads, -0.0 and denormals arrive as they were).
//
// The kernel is a transpose through LDS and nothing else; what it costs is the bytes (6 per S16 sample, 8 per F32 sample).
//   loads   coalesced on the FLAT index of the frame buffer: a wave reads 64 consecutive aligned 4-byte words (non-temporal:
//           the input is used once), whatever nch is.  For S16 a word holds two samples, of two channels or (odd nch) of two
//           frames: each half goes where ITS flat index says, so an odd nch -- frames that start 2-byte aligned -- needs no
//           byte loads.  Only words that hold a wanted sample are read; when nframes * nch is odd the last one is read whole.
//           One word per lane, not 16 bytes: a lane's 4 (8) elements belong to 4 (8) cells of the transposed image, so wider
//           loads buy no fewer LDS writes, and with 4 loads in flight per lane a workgroup has 4 KB outstanding either way.
//   LDS     the tile TRANSPOSED, [channel][SC] words, the S16 samples already converted: the stores then read rows linearly
//           (lane l word l: no conflict whatever SC is), and SC only has to spread the WRITES of a 32-lane group over the 32
//           banks a ds_write_b32 sees.
//             wide tile (nch > 64): a write instruction holds one frame of 64 channels, lane l in row l: bank (l * SC + f) % 32,
//               all different for odd SC.  SC = 65.
//             flat tile (nch <= 64): a group holds 32 consecutive flat elements (S16: every second one of 64), i.e. ~32 / nch
//               frames of every channel: bank (c * SC + f) % 32.  SC = TF + ceil(32 / nch) below 32 channels (a channel's
//               frames of a group get a bank range of their own), TF + 1 from there (a group is one frame of 32 channels).  In
//               the bank model that is conflict-free for the powers of two and at most 2-way (F32) / 4-way (S16) for the
//               rest.  A stride searched per channel count for the fewest conflicts measured the same (1 .. 48 channels x
//               262 144 frames, both formats: within the spread of 1-2 us of 15-32 us); even no padding at all, up to 32-way,
//               cost at most 20 % (48 channels): the kernel waits for memory, not for LDS (profiles/LEDGER.md).
//   stores  one wave instruction writes 64 consecutive frames of ONE channel (256 B of its dm row).
//   tiles   nch <= 64 (what a file or a sound card has): all channels x TF = 64 * max(1, 64 / nch) frames, a contiguous span
//           of the buffer of ~4096 elements, so that one channel does not leave 63 of 64 lanes idle: flat index -> (frame,
//           channel) by a multiply-high with ceil(2^32 / nch) from the host (exact below 2^32 / nch; the index is <= 4096).
//           nch > 64: 64 channels x 64 frames (lane = channel while loading, lane = frame while storing: no division at all).
//           Each lane loads the word that holds its sample there, so for S16 two lanes share a word: the same 128 B line per
//           row either way.
// Nothing of dm outside rows [0, nch) x columns [0, nframes) is written, nothing outside the frame buffer is read (above).
// Budget: <= 32 VGPRs, no scratch, dynamic LDS nch * SC * 4 <= 16640 B (either tile; the wide one is 64 * 65 * 4);
// 256 threads, so at least 9 workgroups fit a CU's LDS (tests/test_pcm_host.py reads the counts from the code object).
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "acg_internal.h"

#define PCM_WG 256
#define PCM_WAVES (PCM_WG / 64)
#define PCM_WIDE_SC 65
#define PCM_S16 1       // == ACG_PCM_S16 / ACG_PCM_F32 of the public header
#define PCM_F32 2

struct PcmKArgs {
    const uint32_t* src;        // the frame buffer as aligned 32-bit words
    uint32_t* dm;               // float rows, moved as words
    size_t dm_pitch;
    unsigned int nch, nframes;
    unsigned int tf;            // flat tile: frames per tile (a multiple of 64)
    unsigned int sc;            // LDS row stride in words
    unsigned int magic;         // flat tile: ceil(2^32 / nch); 0 for nch == 1
};

template <int FMT>
__device__ __forceinline__ uint32_t pcm_word(uint32_t v, unsigned int odd)
{
    if (FMT == PCM_F32) return v;
    const int x = (int)(short)(odd ? (v >> 16) : (v & 0xffffu));
    return __float_as_uint((float)x * (1.0f / 32768.0f));
}

__device__ __forceinline__ unsigned int pcm_div(unsigned int x, unsigned int magic)
{
    return magic ? __umulhi(x, magic) : x;
}

template <int FMT>
__device__ __forceinline__ void pcm_deint_flat(const PcmKArgs& a, uint32_t* lds)
{
    const unsigned int t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned int f0 = blockIdx.x * a.tf;
    const unsigned int nf = min(a.tf, a.nframes - f0);
    const unsigned int nel = nf * a.nch;                                        // <= 4096
    const unsigned int nw = FMT == PCM_S16 ? (nel + 1u) >> 1 : nel;             // f0 * nch is even (64 | tf): the span starts on a word
    const size_t e0 = (size_t)f0 * a.nch;
    const uint32_t* src = a.src + (FMT == PCM_S16 ? e0 >> 1 : e0);
    for (unsigned int k0 = 0; k0 < nw; k0 += 4 * PCM_WG) {
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned int w = k0 + u * PCM_WG + t;
            v[u] = w < nw ? __builtin_nontemporal_load(src + w) : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned int w = k0 + u * PCM_WG + t;
            if (w >= nw) continue;
            if (FMT == PCM_F32) {
                const unsigned int f = pcm_div(w, a.magic), c = w - f * a.nch;
                lds[c * a.sc + f] = v[u];
            } else {
#pragma unroll
                for (unsigned int j = 0; j < 2; ++j) {
                    const unsigned int odd = j, el = 2u * w + odd;
                    if (el < nel) {
                        const unsigned int f = pcm_div(el, a.magic), c = el - f * a.nch;
                        lds[c * a.sc + f] = pcm_word<FMT>(v[u], odd);
                    }
                }
            }
        }
    }
    __syncthreads();
    // item i = 64 frames of one channel, channels fastest
    const unsigned int items = a.nch * ((nf + 63u) >> 6);
    for (unsigned int i = wave; i < items; i += PCM_WAVES) {
        const unsigned int chunk = pcm_div(i, a.magic), c = i - chunk * a.nch;
        const unsigned int fr = chunk * 64u + lane;
        if (fr < nf) a.dm[(size_t)c * a.dm_pitch + f0 + fr] = lds[c * a.sc + fr];
    }
}

template <int FMT>
__device__ __forceinline__ void pcm_deint_wide(const PcmKArgs& a, uint32_t* lds)
{
    const unsigned int t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned int c0 = blockIdx.x * 64u, f0 = blockIdx.y * 64u;
    const unsigned int tc = min(64u, a.nch - c0), nf = min(64u, a.nframes - f0);
    for (unsigned int r0 = wave; r0 < nf; r0 += 4 * PCM_WAVES) {
        uint32_t v[4];
        unsigned int odd[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned int r = r0 + u * PCM_WAVES;
            const size_t e = (size_t)(f0 + r) * a.nch + c0 + lane;
            odd[u] = (unsigned int)e & 1u;
            v[u] = (r < nf && lane < tc) ? __builtin_nontemporal_load(a.src + (FMT == PCM_S16 ? e >> 1 : e)) : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned int r = r0 + u * PCM_WAVES;
            if (r < nf && lane < tc) lds[lane * PCM_WIDE_SC + r] = pcm_word<FMT>(v[u], odd[u]);
        }
    }
    __syncthreads();
    if (lane < nf)
        for (unsigned int c = wave; c < tc; c += PCM_WAVES)
            a.dm[(size_t)(c0 + c) * a.dm_pitch + f0 + lane] = lds[c * PCM_WIDE_SC + lane];
}

template <int FMT, bool WIDE>
__global__ __launch_bounds__(PCM_WG) void pcm_deint_kernel(PcmKArgs a)
{
    extern __shared__ uint32_t lds[];
    if (WIDE) pcm_deint_wide<FMT>(a, lds);
    else pcm_deint_flat<FMT>(a, lds);
}

static unsigned int flat_tf(unsigned int nch) { return 64u * (64u / nch ? 64u / nch : 1u); }

// the flat tile's LDS row stride: TF + ceil(32 / nch) below 32 channels, TF + 1 from there (see the head of the file)
static unsigned int flat_sc(unsigned int nch)
{
    return flat_tf(nch) + (nch >= 32 ? 1u : (32u + nch - 1) / nch);
}

extern "C" int acg_launch_pcm_deint(const PcmArgs* p, void* stream)
{
    if (p->nframes <= 0 || p->nch <= 0) return 0;
    if (p->fmt != PCM_S16 && p->fmt != PCM_F32) return (int)hipErrorInvalidValue;
    PcmKArgs a{};
    a.src = (const uint32_t*)p->frames;
    a.dm = (uint32_t*)p->dm;
    a.dm_pitch = p->dm_pitch;
    a.nch = (unsigned int)p->nch;
    a.nframes = (unsigned int)p->nframes;
    hipStream_t s = (hipStream_t)stream;
    if (a.nch <= 64) {
        a.tf = flat_tf(a.nch);
        a.sc = flat_sc(a.nch);
        a.magic = a.nch == 1 ? 0u : (unsigned int)(((1ull << 32) + a.nch - 1) / a.nch);
        const dim3 grid((a.nframes + a.tf - 1) / a.tf);
        const size_t lds = (size_t)a.nch * a.sc * sizeof(uint32_t);
        if (p->fmt == PCM_S16) hipLaunchKernelGGL((pcm_deint_kernel<PCM_S16, false>), grid, dim3(PCM_WG), lds, s, a);
        else hipLaunchKernelGGL((pcm_deint_kernel<PCM_F32, false>), grid, dim3(PCM_WG), lds, s, a);
    } else {
        const unsigned int fy = (a.nframes + 63u) / 64u;
        if (fy > 65535u) return (int)hipErrorInvalidValue;          // (4 M frames per call: max_blocks <= 4096)
        const dim3 grid((a.nch + 63u) / 64u, fy);
        const size_t lds = (size_t)64 * PCM_WIDE_SC * sizeof(uint32_t);
        if (p->fmt == PCM_S16) hipLaunchKernelGGL((pcm_deint_kernel<PCM_S16, true>), grid, dim3(PCM_WG), lds, s, a);
        else hipLaunchKernelGGL((pcm_deint_kernel<PCM_F32, true>), grid, dim3(PCM_WG), lds, s, a);
    }
    return (int)hipGetLastError();
}
