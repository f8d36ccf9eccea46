/*
 * demo_sndfile_wav.c -- sndfile.h (this directory) for RIFF/WAVE PCM16 files, WAVE_FORMAT_EXTENSIBLE included: what the
 * reference's soundfile.c needs to play a recording in an image without libsndfile.  It knows nothing of the GPU or of
 * acarsdec: it opens a file and hands out normalised floats, whole frames only, as libsndfile documents sf_read_float.
 * The chunk walk is wav_frontend.c's.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sndfile.h"

struct sf_private_tag {
	FILE *f;
	int channels;
	sf_count_t frames_left;
};

static uint32_t rd32(const unsigned char *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static unsigned int rd16(const unsigned char *p) { return (unsigned int)(p[0] | (p[1] << 8)); }

SNDFILE *sf_open(const char *path, int mode, SF_INFO *sfinfo)
{
	unsigned char hdr[12], ck[8], fmt[40];
	unsigned int tag = 0, bits = 0, channels = 0;
	int have_fmt = 0, rate = 0;
	SNDFILE *sf;
	FILE *f;

	if (path == NULL || sfinfo == NULL || mode != SFM_READ)
		return NULL;
	f = fopen(path, "rb");
	if (f == NULL)
		return NULL;
	if (fread(hdr, 1, 12, f) != 12 || memcmp(hdr, "RIFF", 4) || memcmp(hdr + 8, "WAVE", 4))
		goto bad;
	while (fread(ck, 1, 8, f) == 8) {
		const uint32_t sz = rd32(ck + 4);
		if (!memcmp(ck, "fmt ", 4)) {
			const uint32_t take = sz < sizeof(fmt) ? sz : (uint32_t)sizeof(fmt);
			memset(fmt, 0, sizeof(fmt));
			if (take < 16 || fread(fmt, 1, take, f) != take)
				goto bad;
			if (fseek(f, (long)(sz - take) + (long)(sz & 1), SEEK_CUR) != 0)
				goto bad;
			tag = rd16(fmt); channels = rd16(fmt + 2); rate = (int)rd32(fmt + 4); bits = rd16(fmt + 14);
			if (tag == 0xFFFE)
				tag = rd16(fmt + 24);              /* WAVE_FORMAT_EXTENSIBLE: the sub-format's first two bytes */
			have_fmt = 1;
		} else if (!memcmp(ck, "data", 4)) {
			if (!have_fmt || tag != 1 || bits != 16 || channels == 0)
				goto bad;
			sf = malloc(sizeof(*sf));
			if (sf == NULL)
				goto bad;
			sf->f = f;
			sf->channels = (int)channels;
			sf->frames_left = (sf_count_t)(sz / (2u * channels));       /* a partial frame at the end is not a frame */
			sfinfo->frames = sf->frames_left;
			sfinfo->samplerate = rate;
			sfinfo->channels = (int)channels;
			sfinfo->format = SF_FORMAT_WAV | SF_FORMAT_PCM_16;
			sfinfo->sections = 1;
			sfinfo->seekable = 1;
			return sf;
		} else if (fseek(f, (long)sz + (long)(sz & 1), SEEK_CUR) != 0) {
			goto bad;
		}
	}
bad:
	fclose(f);
	return NULL;
}

sf_count_t sf_read_float(SNDFILE *sf, float *ptr, sf_count_t items)
{
	unsigned char raw[2 * 1024];
	sf_count_t done = 0, frames;

	if (sf == NULL || ptr == NULL || items <= 0)
		return 0;
	frames = items / sf->channels;
	if (frames > sf->frames_left)
		frames = sf->frames_left;
	while (frames > 0) {
		const size_t fb = 2 * (size_t)sf->channels;
		size_t want = sizeof(raw) / fb, got, i;
		if (want == 0)
			return done;                                                /* more than 1024 channels: not a sound file */
		if ((sf_count_t)want > frames)
			want = (size_t)frames;
		got = fread(raw, fb, want, sf->f);                                  /* whole frames: a file cut short mid-frame ends here */
		for (i = 0; i < got * (size_t)sf->channels; i++)
			ptr[done + (sf_count_t)i] = (float)(int16_t)rd16(raw + 2 * i) / 32768.0f;
		done += (sf_count_t)(got * (size_t)sf->channels);
		frames -= (sf_count_t)got;
		sf->frames_left -= (sf_count_t)got;
		if (got < want) {
			sf->frames_left = 0;
			break;
		}
	}
	return done;
}

int sf_close(SNDFILE *sf)
{
	if (sf == NULL)
		return 1;
	fclose(sf->f);
	free(sf);
	return 0;
}
