/*
 * sndfile_driver.c -- a stand-alone reader on acarsdec_amd/csrc/demo/sndfile.h, for tests/test_pcm_host.py: opens argv[1] the
 * way soundfile.c does, reads it in requests of argv[2] frames and writes the floats to argv[3]; stdout: the SF_INFO fields,
 * then every request's return value.  Built with the sanitizers.
 */
#include <stdio.h>
#include <stdlib.h>
#include "sndfile.h"

int main(int argc, char **argv)
{
	SF_INFO info;
	SNDFILE *sf;
	FILE *out;
	float *buf;
	long req;
	sf_count_t got;

	if (argc != 4)
		return 2;
	info.format = 0;
	sf = sf_open(argv[1], SFM_READ, &info);
	if (sf == NULL) {
		printf("open failed\n");
		return sf_close(NULL) == 0 ? 2 : 1;
	}
	req = atol(argv[2]);
	printf("%d %d %lld\n", info.channels, info.samplerate, (long long)info.frames);
	buf = malloc(sizeof(float) * (size_t)req * (size_t)info.channels);
	out = fopen(argv[3], "wb");
	if (buf == NULL || out == NULL)
		return 2;
	do {
		got = sf_read_float(sf, buf, (sf_count_t)req * info.channels);
		printf("%lld\n", (long long)got);
		fwrite(buf, sizeof(float), (size_t)got, out);
	} while (got != 0);
	got = sf_read_float(sf, buf, (sf_count_t)req * info.channels);        /* past the end: still 0 */
	printf("%lld\n", (long long)got);
	fclose(out);
	free(buf);
	return sf_close(sf);
}
