// tf_ucis.hip.h -- the spin-blocked orbital-rotation matrices A and B of a UHF determinant on the HBM-resident tensor: unrestricted
// CIS / TDHF and the UHF/UHF stability analysis (calculate_A_matrix / calculate_B_matrix, "UHF" branch, tuna_ci.py:755-757, :823-825;
// calculate_unrestricted_single_reference_excited_states, :1377-1455; build_orbital_hessian, :852-915).  Per spin s: occupied window
// [n_frozen_s, n_s) of o_s orbitals, virtual window [n_s, N) of v_s, d_s = o_s v_s; dim = d_a + d_b; compound index: the alpha block
// first, (ia) = i v_a + a, then the beta block, d_a + j v_b + b -- the reference's spin-conserving subset of its energy-sorted spin
// orbitals up to a permutation.  With G = (ia s|jb t), and within one spin H = (ij|ab), X = (ib|ja), Delta = diag(e_a - e_i):
//     A     = d_st (Delta - H) + G              A + B = d_st (Delta - H - X) + 2 G              A - B = d_st (Delta - H + X)
// each symmetrised as 1/2 (M + M^T).  A - B is block-diagonal in spin: its alpha-beta rectangles are written as exact zeros.
// Inputs: (ia|jb) for aa, bb and ab -- g_ab [(ia) alpha][(jb) beta], there is no ba block -- and the transposed (ij|ab) [i][j][a][b]
// for aa and bb (tfcis::transpose_kernel).
//   * uassemble_kernel writes every matrix of the call in one pass over ONE grid of 32 x 32 tiles of [dim][dim]; the spin boundary d_a
//     is generally no multiple of 32, and THE SPIN OF p AND OF q IS PICKED PER ELEMENT, so a tile may hold all four spin pairs.
//     Same spin: as tfcis::assemble_kernel -- G[p][q], X[q][p], Ht at (p, q) are runs along q, read straight into registers; G[q][p],
//     X[p][q], Ht at (q, p) are runs along p, read with p as the lane index into padded LDS tiles and picked up transposed.
//     p alpha, q beta: g_ab[p][q] is a run along q, read directly.  p beta, q alpha: g_ab[q][p] is a run along p, staged through the
//     same padded LDS tile.  Both images of a cross-spin element are the one stored number, so 1/2 (g + g) = g is exact.
//   * Every global read and write is a run of consecutive doubles (broken at most once per row, at d_a); no atomics; out[p][q] and
//     out[q][p] are the same two terms added in either order, so every matrix is symmetric to the last bit.
//   * An empty spin block (o_s = 0 or v_s = 0) has d_s = 0: no element picks it, its pointers are never read.
#pragma once
#include <hip/hip_runtime.h>
#include "tf_cis.hip.h"

namespace tfucis {

// One element before the symmetrisation, in one fixed order of its terms.  kind: 0 = A, 1 = A + B, 2 = A - B
__device__ __forceinline__ double ucis_element(int kind, bool same, double delta, double G, double H, double X)
{
#pragma clang fp contract(off)    // both images of an element round alike wherever the call is inlined
    if (!same) return kind == 0 ? G : (kind == 1 ? 2.0 * G : 0.0);
    switch (kind) {
    case 0: return (delta + G) - H;
    case 1: return ((delta + 2.0 * G) - H) - X;
    default: return (delta - H) + X;
    }
}

struct Spin {
    const double *g;              // [i][a][j][b] = (ia|jb), d x d
    const double *Ht;             // [i][j][a][b] = (ij|ab)
    const double *eps;            // [N] orbital energies of this spin (device)
    int n_frozen, n_occ, o, v;
};

struct AssembleArgs {
    Spin s[2];                    // alpha, beta
    const double *g_ab;           // [(ia) alpha][(jb) beta] = (ia|jb), d_a x d_b
    int n_out;                    // matrices of this call (<= 2)
    int kind[2];
    double *out[2];               // [dim][dim] each
    // TD-DFT / Kohn-Sham stability (tf_tddft_uhf, tf_stability_uks): H and X enter scaled by hfx (Ht may be null when hfx = 0: the block is
    // then neither built nor read), and matrix m gains kfac[m] K after the symmetrisation -- K [dim][dim], the spin-blocked kernel matrix
    // of tf_xckernel.hip.h, is symmetric to the last bit.  The defaults are Hartree-Fock: hfx = 1 multiplies exactly, a null K adds nothing.
    double hfx = 1.0;
    const double *K = nullptr;
    double kfac[2] = {0.0, 0.0};
};

// block (32, 8), grid (dim / 32, dim / 32) rounded up: tile rows p0 .., columns q0 ..
__global__ __launch_bounds__(256) void uassemble_kernel(AssembleArgs A)
{
    __shared__ double sG[TFX_T][TFX_P], sX[TFX_T][TFX_P], sH[TFX_T][TFX_P];     // [q - q0][p - p0]: G[q][p], X[p][q], H at (q, p)
    const long long da = (long long)A.s[0].o * A.s[0].v, db = (long long)A.s[1].o * A.s[1].v, dim = da + db;
    const long long p0 = (long long)blockIdx.y * TFX_T, q0 = (long long)blockIdx.x * TFX_T;
    const int tx = threadIdx.x;
    // ---- the images that run along p: lane index along p
    {
        const long long p = p0 + tx;
        if (p < dim) {
            const int sp = p >= da;
            const long long pl = p - (sp ? da : 0);
            const Spin &S = A.s[sp];
            const int o = S.o, v = S.v;
            const long long d = sp ? db : da;
            const int i = (int)(pl / v), a = (int)(pl - (long long)i * v);
            for (int y = threadIdx.y; y < TFX_T; y += 8) {
                const long long q = q0 + y;
                if (q >= dim) break;
                const int sq = q >= da;
                const long long ql = q - (sq ? da : 0);
                if (sp == sq) {
                    const int j = (int)(ql / v), b = (int)(ql - (long long)j * v);
                    sG[y][tx] = S.g[ql * d + pl];
                    sX[y][tx] = S.g[((long long)i * v + b) * d + (long long)j * v + a];               // (ib|ja)
                    sH[y][tx] = S.Ht ? S.Ht[(((long long)j * o + i) * v + b) * v + a] : 0.0;         // (ji|ba)
                } else if (!sq) {
                    sG[y][tx] = A.g_ab[ql * db + pl];                                                // q alpha, p beta: (q|p)
                }
            }
        }
    }
    __syncthreads();
    // ---- the images that run along q and the output: lane index along q
    const long long q = q0 + tx;
    if (q >= dim) return;
    const int sq = q >= da;
    const long long ql = q - (sq ? da : 0);
    for (int y = threadIdx.y; y < TFX_T; y += 8) {
        const long long p = p0 + y;
        if (p >= dim) break;
        const int sp = p >= da;
        const long long pl = p - (sp ? da : 0);
        if (sp == sq) {
            const Spin &S = A.s[sp];
            const int o = S.o, v = S.v;
            const long long d = sp ? db : da;
            const int i = (int)(pl / v), a = (int)(pl - (long long)i * v);
            const int j = (int)(ql / v), b = (int)(ql - (long long)j * v);
            const double G = S.g[pl * d + ql];
            const double X = sX[tx][y];                                                              // (ib|ja) = X[p][q]
            const double H = S.Ht ? S.Ht[(((long long)i * o + j) * v + a) * v + b] : 0.0;
            const double Gt = sG[tx][y];
            const double Xt = S.g[((long long)j * v + a) * d + (long long)i * v + b];                 // (ja|ib) = X[q][p]
            const double Hq = sH[tx][y];
            const double delta = p == q ? S.eps[S.n_occ + a] - S.eps[S.n_frozen + i] : 0.0;
            const double hH = A.hfx * H, hX = A.hfx * X, hHq = A.hfx * Hq, hXt = A.hfx * Xt;
            for (int m = 0; m < A.n_out; ++m) {
                double r = 0.5 * (ucis_element(A.kind[m], true, delta, G, hH, hX) + ucis_element(A.kind[m], true, delta, Gt, hHq, hXt));
                if (A.K) r += A.kfac[m] * A.K[p * dim + q];
                A.out[m][p * dim + q] = r;
            }
        } else {
            const double G = sp ? sG[tx][y] : A.g_ab[pl * db + ql];                                  // the one stored (alpha|beta) number
            for (int m = 0; m < A.n_out; ++m) {
                const double e = ucis_element(A.kind[m], false, 0.0, G, 0.0, 0.0);
                double r = 0.5 * (e + e);
                if (A.K) r += A.kfac[m] * A.K[p * dim + q];
                A.out[m][p * dim + q] = r;
            }
        }
    }
}

inline void launch_uassemble(const AssembleArgs &A, hipStream_t st)
{
    const long long dim = (long long)A.s[0].o * A.s[0].v + (long long)A.s[1].o * A.s[1].v;
    const unsigned nt = (unsigned)((dim + TFX_T - 1) / TFX_T);
    hipLaunchKernelGGL(uassemble_kernel, dim3(nt, nt), dim3(TFX_T, 8), 0, st, A);
}

}  // namespace tfucis
