// tf_excited_plan.h -- the work space of the excited-state and stability drivers (tf_excited_host.hip.h), stated ONCE: the sections of
// the one array of small device buffers a call carves, the dim^2 arrays its first out-of-memory message counts, and the work space of
// the TDHF reduction.  A driver allocates `total`, takes every pointer from `off` and prints its GB figure from `message`; nothing else
// ties a size to a carve.  No HIP: tests/excited_plan_model compiles it for the CPU, tests/test_excited_plan.py checks it.
// DESIGN.md section 4.5c.
#pragma once
#include <algorithm>
#include <cstddef>

// The small array, in this order (doubles; a section a driver does not use has length 0):
//   w [dim] | w2 [dim] | e [dim] (dsyevd) | stat [2] | eps [spins][N] | D_ia [3][dim] | mu [dim][3] | f [dim] | C_o [N][o] | C_v [N][v] |
//   D C_v [N][v] | D [3][N][N]
// with o, v those of the one spin (restricted) or of the larger spin block (unrestricted: omax, vmax; the buffers serve the spins in
// turn).  The stability drivers have w | e | eps alone.
enum ExcSection { EXC_W, EXC_W2, EXC_E, EXC_STAT, EXC_EPS, EXC_DIA, EXC_MU, EXC_F, EXC_CO, EXC_CV, EXC_DCV, EXC_DIP, EXC_SECTIONS };

struct ExcitedPlan {
    int dim = 0, nk = 0, tda = 0;             // order of the matrices; kept states (the caller's min(n_keep, dim)); tda: tdhf is not allocated
    size_t off[EXC_SECTIONS + 1] = {};        // first double of each section; off[EXC_SECTIONS] = total
    size_t total = 0, square = 0;             // doubles of the small array; dim^2
    size_t kept_rows = 0, tdhf = 0;           // max(1, nk) dim: one of Q | Xk | Yk; the TDHF reduction: dim^2 (triangular products) + 3 kept_rows
    int n_square = 0;                         // dim^2 arrays the first out-of-memory message counts
    size_t message = 0;                       // doubles behind its GB figure: n_square dim^2 + total (+ 3 kept_rows where it counts them)
    double *at(double *small, ExcSection s) const { return small + off[s]; }
};

static inline ExcitedPlan excited_carve(int N, int dim, int nk, int spins, int o, int v, bool solves, bool tda, int n_square, bool kept_in_message)
{
    ExcitedPlan P;
    const size_t n = (size_t)N, d = (size_t)dim;
    P.dim = dim; P.nk = nk; P.tda = tda; P.square = d * d;
    const size_t len[EXC_SECTIONS] = {d, solves ? d : 0, d, solves ? (size_t)2 : 0, (size_t)spins * n, solves ? 3 * d : 0, solves ? 3 * d : 0, solves ? d : 0,
                                      solves ? n * (size_t)o : 0, solves ? n * (size_t)v : 0, solves ? n * (size_t)v : 0, solves ? 3 * n * n : 0};
    for (int s = 0; s < EXC_SECTIONS; ++s) P.off[s + 1] = P.off[s] + len[s];
    P.total = P.off[EXC_SECTIONS]; P.kept_rows = (size_t)std::max(1, nk) * d;
    P.tdhf = solves ? P.square + 3 * P.kept_rows : 0; P.n_square = n_square;
    P.message = (size_t)n_square * P.square + (kept_in_message ? 3 * P.kept_rows : 0) + P.total;
    return P;
}

// tf_cis_rhf / tf_tddft_rhf.  dim^2 arrays: one per multiplicity (CIS: A; TDHF: A + B), TDHF also A - B, and the transposed (ij|ab) until
// the assembly is done.  The message has always counted the last whether or not (ab|ij) is built (it is not without exact exchange), so
// the plan does not ask; it also counts the kept vectors of the reduction, which come later
static inline ExcitedPlan excited_plan_rhf(int N, int o, int v, bool tda, bool singlets, bool triplets, int nk)
{
    return excited_carve(N, o * v, nk, 1, o, v, true, tda, (singlets ? 1 : 0) + (triplets ? 1 : 0) + (tda ? 0 : 2) + 1, !tda);
}

// tf_cis_uhf / tf_tddft_uhf.  dim^2 arrays: A (CIS) or A + B and A - B (TDHF); the (ab|ij) of either spin have a message of their own
static inline ExcitedPlan excited_plan_uhf(int N, int dim, int omax, int vmax, bool tda, int nk)
{
    return excited_carve(N, dim, nk, 2, omax, vmax, true, tda, tda ? 1 : 2, false);
}

// tf_stability_rhf / _rks: the singlet and triplet A + B, A - B and the transposed (ij|ab); tf_stability_uhf / _uks: A + B and A - B
static inline ExcitedPlan excited_plan_stability(int N, int dim, int spins)
{
    return excited_carve(N, dim, 0, spins, 0, 0, false, true, spins == 1 ? 4 : 2, false);
}
