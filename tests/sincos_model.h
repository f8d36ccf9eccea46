// CPU model of the demodulator's device sin/cos (acarsdec_amd/csrc/msk_common.h sincos_tab, table from host_setup.c
// acg_host_sincos_table): the same operations in the same order (fma = one rounding).  Test infrastructure, included by
// tests/sincos_model.c (random phases, worst error) and tests/sincos_products.c (the phases a test's inputs visit); both are built
// with gcc -O2 -ffp-contract=off and linked with acarsdec_amd/csrc/host_setup.c.
#ifndef SINCOS_MODEL_H
#define SINCOS_MODEL_H
#include <math.h>
// the constants as msk_common.h spells them (tests/test_msk_exact_inputs.py compares the two texts)
#define SC_128_OVER_2PI (6.36619772367581382433e-01 * 32.0)
#define SC_2PI_OVER_128_HI (1.57079632673412561417e+00 / 32.0)
#define SC_2PI_OVER_128_LO (6.07710050650619224932e-11 / 32.0)
#define SC_S3 -1.98412698412698412698e-04
#define SC_S2 8.33333333333333333333e-03
#define SC_S1 -1.66666666666666666667e-01
#define SC_C2 -1.38888888888888888889e-03
#define SC_C1 4.16666666666666666667e-02
static double tab[128][2];
void acg_host_sincos_table(double* t);       // the product's own table builder (acarsdec_amd/csrc/host_setup.c, linked in)
static void build(void) { acg_host_sincos_table(&tab[0][0]); }
static inline void sc_tab(double x, double* sn, double* cs) {
    const double kd = rint(x * SC_128_OVER_2PI);
    const int q = (int)kd;
    double r = fma(-kd, SC_2PI_OVER_128_HI, x);
    r = fma(-kd, SC_2PI_OVER_128_LO, r);
    const double cj = tab[q & 127][0], sj = tab[q & 127][1];
    const double z = r * r;
    // sin r - r = r z (S1 + z (S2 + z S3)),  cos r - 1 = z (C0 + z (C1 + z C2))
    double ps = fma(z, SC_S3, SC_S2);
    ps = fma(z, ps, SC_S1);
    const double sm = (r * z) * ps;            // sin r - r
    double pc = fma(z, SC_C2, SC_C1);
    pc = fma(z, pc, -0.5);
    const double cm1 = z * pc;                 // cos r - 1
    const double sr = r + sm;
    // cos p = cj + (cj (cos r - 1) - sj sin r);  sin p = sj + (sj (cos r - 1) + cj sin r)
    const double u = fma(cj, cm1, -(sj * sr));
    const double w = fma(sj, cm1, cj * sr);
    *cs = cj + u;
    *sn = sj + w;
}
#endif
