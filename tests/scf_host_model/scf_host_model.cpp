// TEST INFRASTRUCTURE: tuna_amd/csrc/tf_scf_host.h (the host arithmetic of an SCF iteration) behind a C interface, for
// tests/test_scf_host.py.  The model does with host vectors what run_rhf and run_uhf do on the device: make room, write the error vector
// of the step into the physical slot of the new entry, count it, enter its row of scalar products, solve the Pulay equations.  With
// -DSCF_HOST_MAIN the file is a program of its own that runs the test's sequences once (for a sanitizer build; nothing is loaded into
// Python then).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../tuna_amd/csrc/tf_scf_host.h"

namespace {
struct Model {
    tfscf::DiisHistory H;
    std::vector<std::vector<double>> err;   // error vector by physical slot
    std::vector<int> step_of;               // the step whose vector a physical slot holds
    explicit Model(int depth) : H(depth), err((size_t)depth), step_of((size_t)depth, 0) {}
};
}  // namespace

extern "C" {

// Error vectors of the sequences: a 64-bit linear congruential generator (Knuth's MMIX constants), uniform in [-1/2, 1/2)
void shm_random(uint64_t seed, int n, double *out)
{
    uint64_t x = seed;
    for (int k = 0; k < n; ++k) {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        out[k] = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    }
}

void *shm_new(int max_diis) { return new Model(max_diis); }
void shm_free(void *h) { delete (Model *)h; }
int shm_size(void *h) { return ((Model *)h)->H.n_hist; }

// One iteration.  Returns n, the length of the history the step solved on: slots[n] and steps[n] oldest first (steps = the step each
// of those vectors came from), *slot = the physical slot this step's vector went to, *solved = 1 with coef[n] (logical order), -1
// after a singular system (the history is then empty: shm_size).
int shm_step(void *h, int step, const double *e, int len, int *slot, int *slots, int *steps, double *coef, int *solved)
{
    Model *M = (Model *)h;
    tfscf::DiisHistory &H = M->H;
    H.make_room();
    const int s = H.slot_of(H.n_hist);
    M->err[(size_t)s].assign(e, e + len);
    M->step_of[(size_t)s] = step;
    ++H.n_hist;
    const int n = H.n_hist;
    std::vector<double> row((size_t)n);
    for (int m = 0; m < n; ++m) {
        const std::vector<double> &a = M->err[(size_t)H.slot_of(m)], &b = M->err[(size_t)s];
        double d = 0.0;
        for (int k = 0; k < len; ++k) d += a[(size_t)k] * b[(size_t)k];
        row[(size_t)m] = d;
    }
    H.enter_dots(row.data());
    *slot = s;
    for (int m = 0; m < n; ++m) { slots[m] = H.slot_of(m); steps[m] = M->step_of[(size_t)H.slot_of(m)]; }
    std::vector<double> x;
    *solved = H.solve(x) ? 1 : -1;
    if (*solved == 1) for (int m = 0; m < n; ++m) coef[m] = x[(size_t)m];
    return n;
}

double shm_damping(double max_damping, int n_atoms, int nao0, int nao1, const double *num, const double *den)
{
    tf_scf_opts o = {};
    o.max_damping = max_damping; o.n_atoms = n_atoms; o.n_atom_ao[0] = nao0; o.n_atom_ao[1] = nao1;
    return tfscf::damping_factor_tail(o, num, den);
}

// thr: delta_E, max_DP, rms_DP, commutator
int shm_converged(const double *thr, double dE, double maxDP, double rmsDP, double commutator)
{
    tf_scf_opts o = {};
    o.conv_delta_E = thr[0]; o.conv_max_DP = thr[1]; o.conv_rms_DP = thr[2]; o.conv_commutator = thr[3];
    return tfscf::scf_converged(o, dE, maxDP, rmsDP, commutator) ? 1 : 0;
}

}  // extern "C"

#ifdef SCF_HOST_MAIN
// The sequences of tests/test_scf_host.py (same seeds, lengths and the repeated vector) once each, then the tail and the predicate
int main()
{
    const int depths[7] = {1, 2, 3, 6, 8, 64, 6};
    long long solved_steps = 0, resets = 0;
    for (int c = 0; c < 7; ++c) {
        const int depth = depths[c], len = depth > 32 ? 400 : 40, n_steps = 3 * depth + 20, repeat_at = c == 6 ? 9 : 0;
        void *h = shm_new(depth);
        std::vector<double> e((size_t)len), prev, coef((size_t)depth);
        std::vector<int> slots((size_t)depth), steps((size_t)depth);
        for (int step = 1; step <= n_steps; ++step) {
            shm_random(1000ULL * (uint64_t)(c + 1) + (uint64_t)step, len, e.data());
            if (step == repeat_at) e = prev;
            prev = e;
            int slot = 0, solved = 0;
            const int n = shm_step(h, step, e.data(), len, &slot, slots.data(), steps.data(), coef.data(), &solved);
            if (n < 1 || n > depth || slot < 0 || slot >= depth) { printf("bad history: length %d, slot %d\n", n, slot); return 1; }
            solved_steps += solved == 1; resets += solved == -1;
        }
        shm_free(h);
    }
    const double num[2] = {0.3, -0.1}, den[2] = {0.5, 0.25}, zero_den[2] = {0.5, 0.0}, thr[4] = {1e-6, 1e-5, 1e-6, 1e-4};
    const double f = shm_damping(0.7, 2, 5, 3, num, den), f0 = shm_damping(0.7, 2, 5, 3, num, zero_den);
    if (!(f > 0.0 && f < 0.7) || f0 != 0.0) { printf("bad damping factors %g %g\n", f, f0); return 1; }
    if (!shm_converged(thr, 0.5e-6, 0.5e-5, 0.5e-6, 0.5e-4) || shm_converged(thr, 2e-6, 0.5e-5, 0.5e-6, 0.5e-4)) return 1;
    printf("scf_host_model: %lld solved steps, %lld resets\n", solved_steps, resets);
    return resets == 1 ? 0 : 1;
}
#endif
