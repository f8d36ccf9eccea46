/*
 * acarsdec_amd_compat_pcm.h -- the legacy view's entry point for the front ends that deliver 12.5 kHz samples themselves
 * (soundfile.c; alsa.c has one channel and needs none).  Included by acarsdec_amd_compat.h, which is what a bound front end
 * includes; defined by compat_msk.c like the others, on the reference's globals channel[] and nbch.
 */
#ifndef ACARSDEC_AMD_COMPAT_PCM_H
#define ACARSDEC_AMD_COMPAT_PCM_H

#ifdef __cplusplus
extern "C" {
#endif

/* soundfile.c:71-77: the per-channel de-interleave + demodMSK() loop, for one sf_read_float() result of `nframes` interleaved
 * frames of nbch channels (at most MAXNBFRAMES = 4096 per read in the reference; longer reads work).  One GPU call and one state
 * download for all channels; the bits are replayed through decodeAcars() channel by channel, the order of the loop it replaces. */
void acarsdec_amd_pcm_frames(const float *interleaved, int nframes);

#ifdef __cplusplus
}
#endif
#endif /* ACARSDEC_AMD_COMPAT_PCM_H */
