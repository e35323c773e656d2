// TEST INFRASTRUCTURE: tuna_amd/csrc/tf_cc_diis.h (the host side of the coupled-cluster DIIS) behind a C interface, for
// tests/test_cc_diis.py.  The model does with host vectors what the drivers do on the device: the error vector of a step goes into the
// slot DiisHistory::store() names, the new row of dots is taken over the history as it stands after drop_oldest(), and from step 3 on
// the Pulay equations are solved.  With -DCC_DIIS_MAIN the file is a program of its own that runs the test's sequences once (for a
// sanitizer build; nothing is loaded into Python then).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../tuna_amd/csrc/tf_cc_diis.h"

namespace {
struct Model {
    tfccd::DiisHistory D;
    std::vector<std::vector<double>> err;   // error vector by slot
    std::vector<int> step_of;               // the step whose vector a slot holds
};
}  // namespace

extern "C" {

// Error vectors of the sequences: a 64-bit linear congruential generator (Knuth's MMIX constants), uniform in [-1/2, 1/2)
void ccdm_random(uint64_t seed, int n, double *out)
{
    uint64_t x = seed;
    for (int k = 0; k < n; ++k) {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        out[k] = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    }
}

void *ccdm_new(int use_diis, int max_diis)
{
    Model *M = new Model;
    M->D.init(use_diis != 0, max_diis);
    M->err.resize((size_t)M->D.nslot);
    M->step_of.assign((size_t)M->D.nslot, 0);
    return M;
}

void ccdm_free(void *h) { delete (Model *)h; }
int ccdm_keep(void *h) { return ((Model *)h)->D.keep; }
int ccdm_nslot(void *h) { return ((Model *)h)->D.nslot; }
int ccdm_size(void *h) { return (int)((Model *)h)->D.order.size(); }

// One storing step.  Returns n, the length of the history the step worked on (after the drop): slots[n] and steps[n] oldest first
// (steps = the step each of those vectors came from), *slot = where this step's vector went, *solved = 1 with coef[n] (history
// order), 0 before step 3, -1 after a singular system (the history is then empty: ccdm_size).
int ccdm_step(void *h, int step, const double *e, int len, int *slot, int *slots, int *steps, double *coef, int *solved)
{
    Model *M = (Model *)h;
    tfccd::DiisHistory &D = M->D;
    const int s = D.store();
    M->err[(size_t)s].assign(e, e + len);
    M->step_of[(size_t)s] = step;
    D.drop_oldest(step);
    const int n = (int)D.order.size();
    std::vector<double> row((size_t)n);
    for (int m = 0; m < n; ++m) {
        const std::vector<double> &a = M->err[(size_t)D.order[(size_t)m]], &b = M->err[(size_t)s];
        double d = 0.0;
        for (int k = 0; k < len; ++k) d += a[(size_t)k] * b[(size_t)k];
        row[(size_t)m] = d;
    }
    D.enter_dots(s, row.data());
    *slot = s;
    for (int m = 0; m < n; ++m) { slots[m] = D.order[(size_t)m]; steps[m] = M->step_of[(size_t)D.order[(size_t)m]]; }
    *solved = 0;
    if (step > 2) *solved = D.solve(coef) ? 1 : -1;
    return n;
}

}  // extern "C"

#ifdef CC_DIIS_MAIN
// The sequences of tests/test_cc_diis.py (same seeds, lengths and the repeated vector), once each
int main()
{
    const int len = 40, depths[6] = {1, 2, 3, 6, 32, 40};
    long long solved_steps = 0, resets = 0;
    for (int c = 0; c < 7; ++c) {
        const int max_diis = c < 6 ? depths[c] : 6, n_steps = 70, repeat_at = c < 6 ? 0 : 9;
        void *h = ccdm_new(1, max_diis);
        std::vector<double> e((size_t)len), prev, coef(33);
        std::vector<int> slots(33), steps(33);
        for (int step = 1; step <= n_steps; ++step) {
            ccdm_random(1000ULL * (uint64_t)(c + 1) + (uint64_t)step, len, e.data());
            if (step == repeat_at) e = prev;
            prev = e;
            int slot = 0, solved = 0;
            const int n = ccdm_step(h, step, e.data(), len, &slot, slots.data(), steps.data(), coef.data(), &solved);
            if (n < 1 || n > ccdm_nslot(h)) { printf("bad history length %d\n", n); return 1; }
            solved_steps += solved == 1; resets += solved == -1;
        }
        ccdm_free(h);
    }
    void *off = ccdm_new(0, 6);
    if (ccdm_nslot(off) != 0) return 1;
    ccdm_free(off);
    printf("cc_diis_model: %lld solved steps, %lld resets\n", solved_steps, resets);
    return resets == 1 ? 0 : 1;
}
#endif
