// TEST INFRASTRUCTURE: the HIP-free work-space plan of the excited-state and stability drivers (tuna_amd/csrc/tf_excited_plan.h) behind a
// C interface for tests/test_excited_plan.py.  No GPU code.
#include "../../tuna_amd/csrc/tf_excited_plan.h"

// out = {off[0 .. EXC_SECTIONS] (the last is the end of the last section), total, square, n_square, kept_rows, tdhf, message, tda}
static void put(const ExcitedPlan &P, long long *out)
{
    for (int s = 0; s <= EXC_SECTIONS; ++s) out[s] = (long long)P.off[s];
    long long *q = out + EXC_SECTIONS + 1;
    q[0] = (long long)P.total; q[1] = (long long)P.square; q[2] = P.n_square; q[3] = (long long)P.kept_rows; q[4] = (long long)P.tdhf;
    q[5] = (long long)P.message; q[6] = P.tda ? 1 : 0;
}

extern "C" {

int excm_sections(void) { return EXC_SECTIONS; }

void excm_rhf(int N, int o, int v, int tda, int singlets, int triplets, int nk, long long *out)
{
    put(excited_plan_rhf(N, o, v, tda != 0, singlets != 0, triplets != 0, nk), out);
}

void excm_uhf(int N, int dim, int omax, int vmax, int tda, int nk, long long *out) { put(excited_plan_uhf(N, dim, omax, vmax, tda != 0, nk), out); }

void excm_stability(int N, int dim, int spins, long long *out) { put(excited_plan_stability(N, dim, spins), out); }

}
