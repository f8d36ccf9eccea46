// state.cpp -- a context's state read and written from the host: bit log, dm image, channel state, block text, and the lab
// presets of the block and stream counters.
#include "acg_ctx.h"

extern "C" int acg_read_bits(acg_ctx* ctx, int ch, float* vo, float* lvl, int max_bits, int* nbits)
{
    if (!ctx || !nbits || ch < 0 || ch >= ctx->cfg.nch) return ACG_EINVAL;
    if (!ctx->d_bits) return fail(ctx, ACG_ESTATE, "context created without ACG_F_BITLOG");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    int n = 0;
    HIPCHK(ctx, hipMemcpy(&n, ctx->d_nbits + ch, sizeof(int), hipMemcpyDeviceToHost));
    *nbits = n;
    const int m = std::min(std::min(n, ctx->bit_cap), max_bits);
    if (m > 0) {
        std::vector<float2> tmp((size_t)m);
        HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->d_bits + (size_t)ch * ctx->bit_cap, (size_t)m * sizeof(float2),
                              hipMemcpyDeviceToHost));
        for (int i = 0; i < m; ++i) {
            if (vo) vo[i] = tmp[(size_t)i].x;
            if (lvl) lvl[i] = tmp[(size_t)i].y;
        }
    }
    return n > ctx->bit_cap ? ACG_EOVERFLOW : ACG_OK;
}

extern "C" int acg_read_bits_all(acg_ctx* ctx, int* counts, float* vo, float* lvl)
{
    if (!ctx || !counts) return ACG_EINVAL;
    if (!ctx->d_bits) return fail(ctx, ACG_ESTATE, "context created without ACG_F_BITLOG");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const size_t nch = (size_t)ctx->cfg.nch, cap = (size_t)ctx->bit_cap;
    HIPCHK(ctx, hipMemcpy(counts, ctx->d_nbits, nch * sizeof(int), hipMemcpyDeviceToHost));
    if (vo || lvl) {
        std::vector<float2> tmp(nch * cap);
        HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->d_bits, tmp.size() * sizeof(float2), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < nch; ++c) {
            const size_t m = (size_t)std::min<int>(counts[c], (int)cap);
            for (size_t i = 0; i < m; ++i) {
                if (vo) vo[c * cap + i] = tmp[c * cap + i].x;
                if (lvl) lvl[c * cap + i] = tmp[c * cap + i].y;
            }
        }
    }
    return ACG_OK;
}

extern "C" int acg_replay_bits(acg_ctx* ctx, acg_bit_sink sink, void* user)
{
    if (!ctx || !sink) return ACG_EINVAL;
    if (!ctx->d_bits) return fail(ctx, ACG_ESTATE, "context created without ACG_F_BITLOG");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const size_t nch = (size_t)ctx->cfg.nch, cap = (size_t)ctx->bit_cap;
    std::vector<int> counts(nch);
    HIPCHK(ctx, hipMemcpy(counts.data(), ctx->d_nbits, nch * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float2> tmp(nch * cap);
    HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->d_bits, tmp.size() * sizeof(float2), hipMemcpyDeviceToHost));
    int rc = ACG_OK;
    for (size_t c = 0; c < nch; ++c) {
        if (counts[c] > (int)cap) rc = ACG_EOVERFLOW;
        const size_t m = (size_t)std::min<int>(counts[c], (int)cap);
        for (size_t i = 0; i < m; ++i) sink(user, (int)c, tmp[c * cap + i].x, tmp[c * cap + i].y);
    }
    return rc;
}

extern "C" int acg_read_dm_n(acg_ctx* ctx, int ch0, int n, float* dm, size_t pitch_floats, int nfloats)
{
    if (!ctx || !dm || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch || nfloats < 0 || nfloats > ctx->max_len ||
        (n > 1 && pitch_floats < (size_t)nfloats))
        return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (nfloats)
        HIPCHK(ctx, hipMemcpy2D(dm, pitch_floats * sizeof(float), ctx->d_dm + (size_t)ch0 * ctx->dm_pitch, ctx->dm_pitch * sizeof(float),
                                (size_t)nfloats * sizeof(float), (size_t)n, hipMemcpyDeviceToHost));
    return ACG_OK;
}

extern "C" int acg_read_dm(acg_ctx* ctx, int ch, float* dm, int n)
{
    return acg_read_dm_n(ctx, ch, 1, dm, (size_t)(n > 0 ? n : 0), n);
}

static void state_from_dev(const AcgChan& d, acg_chan_state* st)
{
    st->MskPhi = d.phi; st->MskDf = d.df; st->MskLvlSum = d.lvlsum; st->MskClk = d.clk;
    st->MskBitCount = d.bitcount; st->MskS = d.S; st->idx = d.idx;
    std::memcpy(st->inb, d.inb, sizeof(d.inb));
    st->outbits = (int)d.outbits; st->nbits = d.nbits; st->Acarsstate = d.astate;
    st->blk_len = d.blen; st->blk_err = d.berr;
    // the SOH stamp as a distance (the sample counter is the slot's own, the distance travels): ADVICE r05
    const unsigned int back = (unsigned int)d.nsamp_total - d.soh32;
    st->soh_back = (d.astate >= 3 && d.astate <= 5 && back < 65536u) ? (int)back : 0;
}

// channels ch0 .. ch0+n-1 in one transfer (the legacy view moves all channels of a dongle per callback)
extern "C" int acg_get_state_n(acg_ctx* ctx, int ch0, int n, acg_chan_state* st)
{
    if (!ctx || !st || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    std::vector<AcgChan> d((size_t)n);
    HIPCHK(ctx, hipMemcpy(d.data(), ctx->d_st + ch0, (size_t)n * sizeof(AcgChan), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) state_from_dev(d[(size_t)i], st + i);
    return ACG_OK;
}

extern "C" int acg_get_state(acg_ctx* ctx, int ch, acg_chan_state* st) { return acg_get_state_n(ctx, ch, 1, st); }

extern "C" int acg_set_state_n(acg_ctx* ctx, int ch0, int n, const acg_chan_state* st)
{
    if (!ctx || !st || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch) return ACG_EINVAL;
    for (int i = 0; i < n; ++i) {
        if (st[i].idx >= ACG_FLEN) return fail(ctx, ACG_EINVAL, "idx out of range");
        // blk_len indexes the channel's 256-byte text row on the device (acars.c:304 `blk->txt[blk->len] = r`; the reference resets a
        // block beyond 240 bytes, acars.c:336): a length no decodeAcars() leaves behind is refused instead of written through
        if (st[i].blk_len < 0 || st[i].blk_len > 241) return fail(ctx, ACG_EINVAL, "blk_len out of range");
    }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    // read-modify-write: the bookkeeping that is not part of channel_t (bit / sample counters, the held CRC byte) stays as the
    // device has it; the SOH stamp is re-based on this slot's sample counter from the distance the caller brings
    std::vector<AcgChan> dv((size_t)n);
    HIPCHK(ctx, hipMemcpy(dv.data(), ctx->d_st + ch0, (size_t)n * sizeof(AcgChan), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        AcgChan& d = dv[(size_t)i];
        const acg_chan_state& t = st[i];
        d.phi = t.MskPhi; d.df = t.MskDf; d.lvlsum = t.MskLvlSum; d.clk = t.MskClk;
        d.bitcount = t.MskBitCount; d.S = t.MskS; d.idx = t.idx;
        std::memcpy(d.inb, t.inb, sizeof(d.inb));
        d.outbits = (unsigned int)t.outbits & 0xffu; d.nbits = t.nbits; d.astate = t.Acarsstate;
        d.blen = t.blk_len; d.berr = t.blk_err;
        d.soh32 = (unsigned int)d.nsamp_total - (unsigned int)(t.soh_back > 0 && t.soh_back < 65536 ? t.soh_back : 0);
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_st + ch0, dv.data(), (size_t)n * sizeof(AcgChan), hipMemcpyHostToDevice));
    return ACG_OK;
}

extern "C" int acg_set_state(acg_ctx* ctx, int ch, const acg_chan_state* st) { return acg_set_state_n(ctx, ch, 1, st); }

// blk->txt being assembled (the device keeps 256 bytes per channel, ACG_TXTMAX of them are the reference's msgblk_t::txt)
extern "C" int acg_get_block_text(acg_ctx* ctx, int ch, unsigned char* txt)
{
    if (!ctx || !txt || ch < 0 || ch >= ctx->cfg.nch) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(txt, ctx->d_txt + (size_t)ch * 256, ACG_TXTMAX, hipMemcpyDeviceToHost));
    return ACG_OK;
}

extern "C" int acg_set_block_text(acg_ctx* ctx, int ch, const unsigned char* txt)
{
    if (!ctx || !txt || ch < 0 || ch >= ctx->cfg.nch) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(ctx->d_txt + (size_t)ch * 256, txt, ACG_TXTMAX, hipMemcpyHostToDevice));
    return ACG_OK;
}

// ---- lab: the block counters next to their wrap (acarsdec_amd_lab.h) ----------------------------------------------------
extern "C" int acg_lab_set_block_counter(acg_ctx* ctx, unsigned int value)
{
    if (!ctx) return ACG_EINVAL;
    if (ctx->call_seq != 0) return fail(ctx, ACG_ESTATE, "acg_lab_set_block_counter: only right after acg_reset");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(ctx->d_frame_count, &value, sizeof(value), hipMemcpyHostToDevice));
    if (ctx->d_rep_upto) HIPCHK(ctx, hipMemcpy(ctx->d_rep_upto, &value, sizeof(value), hipMemcpyHostToDevice));
    for (int i = 0; i < acg_ctx::NCALL; ++i) ctx->h_call_count[i] = value;
    ctx->consumed = value;
    HIPCHK(ctx, hipDeviceSynchronize());
    return ACG_OK;
}
extern "C" unsigned int acg_lab_block_ring_size(const acg_ctx* ctx) { return ctx ? ctx->frame_cap : 0u; }

// ---- lab: the stream counters after days of uptime (acarsdec_amd_lab.h) -------------------------------------------------
extern "C" int acg_lab_set_stream_counters(acg_ctx* ctx, int ch0, int n, long long nsamp_total, long long nbit_total)
{
    if (!ctx || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch || nsamp_total < 0 || nbit_total < 0) return ACG_EINVAL;
    if (ctx->call_seq != 0) return fail(ctx, ACG_ESTATE, "acg_lab_set_stream_counters: only right after acg_reset");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    // read-modify-write, as acg_set_state_n: everything but the three counters stays as the device has it
    std::vector<AcgChan> dv((size_t)n);
    HIPCHK(ctx, hipMemcpy(dv.data(), ctx->d_st + ch0, (size_t)n * sizeof(AcgChan), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        AcgChan& d = dv[(size_t)i];
        d.nsamp_total = nsamp_total;
        d.nbit_total = nbit_total;
        d.soh32 = (unsigned int)nsamp_total;
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_st + ch0, dv.data(), (size_t)n * sizeof(AcgChan), hipMemcpyHostToDevice));
    return ACG_OK;
}
