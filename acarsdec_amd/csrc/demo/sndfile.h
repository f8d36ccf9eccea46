/*
 * sndfile.h -- the part of libsndfile's documented API that the reference's soundfile.c uses, for the demo build of an image
 * without libsndfile (demo_sndfile_wav.c implements it for RIFF/WAVE PCM16 files).  Written from the library's API
 * documentation: names, argument order and value conventions are libsndfile's; nothing else is.
 */
#ifndef SNDFILE_H
#define SNDFILE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sf_private_tag SNDFILE;
typedef int64_t sf_count_t;

typedef struct SF_INFO {
	sf_count_t frames;
	int samplerate;
	int channels;
	int format;
	int sections;
	int seekable;
} SF_INFO;

enum { SFM_READ = 0x10 };                        /* reading only: soundfile.c's DEBUG half (sf_write_float) is not served */
enum { SF_FORMAT_WAV = 0x010000, SF_FORMAT_PCM_16 = 0x0002 };

/* opens `path`; SFM_READ fills *sfinfo from the file (its format field must be 0 on entry).  NULL on failure. */
SNDFILE *sf_open(const char *path, int mode, SF_INFO *sfinfo);
/* reads up to `items` samples (a multiple of the channel count) as floats, PCM16 normalised to [-1, 1) by 1/32768;
 * returns the samples read: whole frames only, fewer than asked for at the end of the data, then 0 */
sf_count_t sf_read_float(SNDFILE *sndfile, float *ptr, sf_count_t items);
int sf_close(SNDFILE *sndfile);

#ifdef __cplusplus
}
#endif
#endif /* SNDFILE_H */
