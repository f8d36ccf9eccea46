// The mixer products of the device's sin/cos model (sincos_model.h) against the oracle's, at given (phase, sample) pairs.  Test
// infrastructure: tests/msk_exact_inputs.py builds a shared object from this file and acarsdec_amd/csrc/host_setup.c
// (gcc -O2 -ffp-contract=off) and hands it the phases the oracle visits on the inputs of tests/test_gpu_msk_exact.py.
#include <complex.h>
#include <string.h>
#include "sincos_model.h"

// the model's sin/cos themselves, for a comparison with the device's doubles (acg_selftest_sincos)
void sc_eval(const double* p, double* sn, double* cs, long n)
{
    static int ready;
    if (!ready) { build(); ready = 1; }
    for (long i = 0; i < n; i++) sc_tab(p[i], &sn[i], &cs[i]);
}

// how many of the 2 n float products (float)(in * cos p), (float)(in * -sin p) of sc_tab differ, as bit patterns, from what
// oracle/acars_oracle.c keeps of `in * cexp(-p * I)` (msk.c:90); *first = the index of the first pair with a difference, or -1
long sc_products_differ(const double* p, const float* in, long n, long* first)
{
    static int ready;
    long bad = 0;
    if (!ready) { build(); ready = 1; }
    *first = -1;
    for (long i = 0; i < n; i++) {
        const float complex x = in[i] * cexp(-p[i] * I);
        const float want[2] = {crealf(x), cimagf(x)};
        double s, c;
        sc_tab(p[i], &s, &c);
        const double d = (double)in[i];
        const float got[2] = {(float)(d * c), (float)(d * (-s))};
        const int k = (memcmp(&want[0], &got[0], 4) != 0) + (memcmp(&want[1], &got[1], 4) != 0);
        if (k && *first < 0) *first = i;
        bad += k;
    }
    return bad;
}
