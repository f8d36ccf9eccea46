/* flight_import_driver.c -- the argument checks of acg_flights_import and its neighbours (acg_api.cpp) in a build with
 * -fsanitize=address,undefined, the way tests/sanitize/host_driver.c exercises the rest of the host side: no GPU, the kernel
 * launchers stubbed, nothing here may reach them.  acg_flights_import checks its events with acg_flight_events_check before it
 * looks at the context, so every rule is reachable without one. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "acarsdec_amd.h"

#define STUB(name) int name() { fprintf(stderr, "launcher " #name " reached without a GPU\n"); abort(); return -1; }
STUB(acg_launch_fir) STUB(acg_launch_fir_generic) STUB(acg_launch_fir_shared) STUB(acg_launch_regroup_taps)
STUB(acg_launch_fir_fmt) STUB(acg_launch_msk) STUB(acg_launch_msk2) STUB(acg_launch_blk_repair) STUB(acg_launch_sincos_selftest)
STUB(acg_launch_div2_selftest) STUB(acg_launch_msg_split) STUB(acg_launch_synth_iq) STUB(acg_launch_fill_random) STUB(acg_launch_read_probe)
STUB(acg_fir_mm_takes) STUB(acg_launch_fir_mm_prep) STUB(acg_launch_fir_mm)
STUB(acg_fir_mm1_takes) STUB(acg_launch_fir_mm1_prep) STUB(acg_launch_fir_mm1)
size_t acg_fir_mm1_image_bytes() { return 0; }
size_t acg_fir_lds_bytes() { return 0; }
size_t acg_fir_mm_image_bytes() { return 0; }

static int fails;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static acg_flight_event good(int i)
{
	acg_flight_event e;
	memset(&e, 0, sizeof(e));
	e.end_sample = 30000 + 17ll * i;
	e.soh_sample = e.end_sample - 900;
	e.sec = 1700000000;
	e.usec = (i * 80) % 1000000;
	e.chn = i % 64;
	memcpy(e.addr, "N12345", 6);
	memcpy(e.fid, "XY0001", 6);
	e.e_ok = (char)(i & 1);
	return e;
}

int main(void)
{
	enum { N = 700 };
	/* heap arrays of exactly n records: a check that reads past the n-th is an AddressSanitizer report */
	acg_flight_event *ev = malloc(N * sizeof(*ev)), *one = malloc(sizeof(*one));
	int i, n = -1;
	CHECK(sizeof(acg_flight_event) == 88);
	for (i = 0; i < N; ++i)
		ev[i] = good(i);
	CHECK(acg_flight_events_check(ev, N) == ACG_OK && acg_flight_events_check(ev, 0) == ACG_OK && acg_flight_events_check(NULL, 0) == ACG_OK);
	CHECK(acg_flight_events_check(NULL, 1) == ACG_EINVAL && acg_flight_events_check(ev, -1) == ACG_EINVAL);
	/* the limits themselves pass */
	*one = good(1); one->usec = 0; CHECK(acg_flight_events_check(one, 1) == ACG_OK);
	*one = good(1); one->usec = 999999; CHECK(acg_flight_events_check(one, 1) == ACG_OK);
	*one = good(1); one->chn = (1 << 20) - 1; CHECK(acg_flight_events_check(one, 1) == ACG_OK);
	*one = good(1); one->end_sample = (1ll << 43) - 1; CHECK(acg_flight_events_check(one, 1) == ACG_OK);
	*one = good(1); one->end_sample = 0; one->soh_sample = -5000; one->sec = -1; one->fid[0] = 0; CHECK(acg_flight_events_check(one, 1) == ACG_OK);
	/* each rule, alone */
	*one = good(1); one->usec = -1; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->usec = 1000000; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->addr[0] = 0; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->chn = -1; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->chn = 1 << 20; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->end_sample = -1; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->end_sample = 1ll << 43; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->e_ok = 2; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	*one = good(1); one->e_ok = (char)-1; CHECK(acg_flight_events_check(one, 1) == ACG_EINVAL);
	/* one bad record anywhere refuses the whole array: the first, one in the middle, the last */
	for (i = 0; i < 3; ++i) {
		const int at = i == 0 ? 0 : i == 1 ? N / 2 : N - 1;
		const acg_flight_event keep = ev[at];
		ev[at].usec = 1000000;
		CHECK(acg_flight_events_check(ev, N) == ACG_EINVAL);
		CHECK(acg_flight_events_check(ev, at) == ACG_OK);              /* (the records before it are fine) */
		ev[at] = keep;
	}
	CHECK(acg_flight_events_check(ev, N) == ACG_OK);
	/* the entry points: no context, nothing to queue at */
	CHECK(acg_flights_import(NULL, ev, N) == ACG_EINVAL && acg_flights_import(NULL, NULL, 0) == ACG_EINVAL);
	CHECK(acg_flights_set_channels(NULL, NULL) == ACG_EINVAL && acg_flights_export(NULL, 1) == ACG_EINVAL);
	CHECK(acg_drain_flight_events(NULL, ev, N, &n) == ACG_EINVAL && n == -1);
	CHECK(acg_flights_commit(NULL) == ACG_EINVAL);
	free(ev);
	free(one);
	if (fails) {
		fprintf(stderr, "%d check(s) failed\n", fails);
		return 1;
	}
	puts("sanitized flight import driver: ok");
	return 0;
}
