// tf_dft_plan.h -- the device buffers of the Kohn-Sham grid and the split of the V_XC contraction, stated ONCE: which buffers a grid
// owns and how long each is, where the split-K partials of V = Phi^T D and their sum lie, and the owner that allocates a set of buffers
// whole or not at all and frees each exactly once.  tf_dft.hip.h takes the constants from here (the kernels see the same values),
// tf_dft_host.hip.h everything else.  No HIP: tests/dft_plan_model compiles it for the CPU, tests/test_dft_plan.py checks it.
// DESIGN.md section 4.6d.
#pragma once
#include <cstddef>

namespace tfdft {

// V = Phi^T D contracts over ~10^5 grid points into an N x N matrix: as ONE GEMM rocBLAS runs it in a single workgroup (4.7 ms for CO /
// def2-TZVP); split over the grid points into VSPLIT batch entries it fills the GPU, and the partials are added in fixed order.
const int VSPLIT = 128;            // (512 partials of 200 grid points each cost more to add up -- 0.18 ms -- than the GEMM they split)
const int NPART = 512;             // blocks of the reduction kernels: partial sums of the integrals, added on the host in block order
// per-point rows of the spin set's pt ([SPT][G]): 0-1 rho_a, rho_b (raw, then floored); 2-4, 5-7 grad rho_a, grad rho_b; 8-9 v_rho_a, v_rho_b;
// 10-12, 13-15 c_a, c_b; 16-18 e_X,a rho_a, e_X,b rho_b, e_C rho
const int SPT = 19;

// The split of a contraction over G grid points into an output of `width` doubles (N N restricted, 2 N N with both spins side by side):
// VSPLIT parts of Kc points each (none if G < VSPLIT), then one part of the rem points from point `first_rem` on; part s is written to
// buf + part_off(s), their sum in part order to buf + sum_off().  The buffer has VSPLIT + 2 slots: the sum slot lies behind the last
// slot a partial can take (slot VSPLIT, the remainder's when Kc > 0).
struct SplitPlan {
    long long Kc = 0, rem = 0, first_rem = 0, width = 0;
    int nparts = 0, rem_slot = 0;                        // parts written; the remainder's slot (meaningful if rem > 0)
    long long part_off(int s) const { return (long long)s * width; }
    long long sum_off() const { return (long long)(VSPLIT + 1) * width; }
};
static inline size_t split_doubles(size_t width) { return (size_t)(VSPLIT + 2) * width; }
static inline SplitPlan split_plan(long long G, long long width)
{
    SplitPlan S;
    S.Kc = G / VSPLIT; S.rem = G - S.Kc * VSPLIT; S.first_rem = S.Kc * VSPLIT; S.width = width;
    S.rem_slot = S.Kc > 0 ? VSPLIT : 0;
    S.nparts = S.rem_slot + (S.rem > 0 ? 1 : 0);
    return S;
}

// The base set, in allocation order (doubles):
//   w [G] | phi [G][N] | dphi [3][G][N] (LDA: [1][G][N], never read) | B [G][N] | D [G][N] | rho [G] | grad [3][G] | vrho [G] | vsig [G] |
//   ex [G] | ec [G] | V [VSPLIT + 2][N][N] (SplitPlan) | part [NPART][3]
enum GridBuf { GB_W, GB_PHI, GB_DPHI, GB_B, GB_D, GB_RHO, GB_GRAD, GB_VRHO, GB_VSIG, GB_EX, GB_EC, GB_V, GB_PART, GB_COUNT };
static inline void grid_base_lengths(long long G_, int N_, bool gga, size_t len[GB_COUNT])
{
    const size_t G = (size_t)G_, N = (size_t)N_;
    const size_t l[GB_COUNT] = {G, G * N, (gga ? 3 : 1) * G * N, G * N, G * N, G, 3 * G, G, G, G, G, split_doubles(N * N), (size_t)3 * NPART};
    for (int k = 0; k < GB_COUNT; ++k) len[k] = l[k];
}

// The spin set of the unrestricted path, allocated on its first use, both spins side by side in every row:
//   P [N][2N] packed P_alpha | P_beta | B [G][2N] | D [G][2N] | pt [SPT][G] | V [VSPLIT + 2][N][2N] | part [NPART][5] |
//   io [4][N][N] host <-> device staging (P_alpha, P_beta, V_alpha, V_beta)
enum SpinBuf { GS_P, GS_B, GS_D, GS_PT, GS_V, GS_PART, GS_IO, GS_COUNT };
static inline void grid_spin_lengths(long long G_, int N_, size_t len[GS_COUNT])
{
    const size_t G = (size_t)G_, N = (size_t)N_, nn = N * N;
    const size_t l[GS_COUNT] = {2 * nn, G * 2 * N, G * 2 * N, (size_t)SPT * G, split_doubles(2 * nn), (size_t)5 * NPART, 4 * nn};
    for (int k = 0; k < GS_COUNT; ++k) len[k] = l[k];
}

// Owner of one set of buffers.  acquire() asks `alloc` (0: success) for count blocks of len[k] doubles in the order of the list; at the
// first refusal it frees what it got, leaves p as it was (all null) and returns alloc's code.  release() frees each block once.
typedef int (*GridAllocFn)(void **p, size_t bytes);
typedef void (*GridFreeFn)(void *p);
struct GridBlocks {
    static const int MAX = (int)GB_COUNT > (int)GS_COUNT ? (int)GB_COUNT : (int)GS_COUNT;
    double *p[MAX] = {};
    int count = 0;
    GridFreeFn free_fn = nullptr;
    bool held() const { return count > 0; }
    int acquire(const size_t *len, int n, GridAllocFn alloc, GridFreeFn fr)
    {
        if (held() || n > MAX) return -1;
        double *got[MAX] = {};
        for (int k = 0; k < n; ++k) {
            const int rc = alloc((void **)&got[k], len[k] * sizeof(double));
            if (rc != 0) {
                for (int q = 0; q < k; ++q) fr(got[q]);
                return rc;
            }
        }
        for (int k = 0; k < n; ++k) p[k] = got[k];
        count = n; free_fn = fr;
        return 0;
    }
    void release()
    {
        for (int k = 0; k < count; ++k) { free_fn(p[k]); p[k] = nullptr; }
        count = 0;
    }
};

// The grid of a context: G > 0 exactly when the base set is held whole and the AOs are on it (tf_dft_setup commits nothing less)
struct Grid {
    long long G = 0;
    int N = 0, xid = 0, cid = 0;
    bool gga = false;
    double dfx = 0, dfc = 0, x_alpha = 2.0 / 3.0;
    GridBlocks base, spin;
    double *b(GridBuf k) const { return base.p[k]; }
    double *s(SpinBuf k) const { return spin.p[k]; }
};

inline void release(Grid &g)
{
    g.base.release();
    g.spin.release();
    g = Grid();
}

}  // namespace tfdft
