// tf_mp2dens.hip.h -- the restricted MP2 one-particle density on the HBM-resident tensor: unrelaxed, and relaxed through the Z-vector
// equations (run_restricted_MP2, tuna_mp.py:908-966; calculate_restricted_relaxed_MP2_density_matrix, :177-279).
// Notation of tf_mp3.hip.h / tf_mp4.hip.h: occupied window i, j, k (o orbitals), virtual window a, b, c (v orbitals),
// D = e_i + e_j - e_a - e_b, and with the weights c_os, c_ss of the opposite- and same-spin parts (1, 1: MP2)
//     tOS_ijab = -2 (ia|jb) / D,   tSS_ijab = [(ia|jb) - (ib|ja)] / D,   w_ijab = c_os 2 (ia|jb) / D + c_ss 2 [(ia|jb) - (ib|ja)] / D.
// Unrelaxed (GEMMs of the caller over T[i][a][j][b] = t_ijab, read as [o][(v o v)] and as [(o v o)][v]; t_kiab = t_ikba):
//     P_ij = -1/2 c_os sum_kab tOS_kiab tOS_kjab - c_ss sum_kab tSS_kiab tSS_kjab,
//     P_ab = +1/2 c_os sum_ijc tOS_ijbc tOS_ijac + c_ss sum_ijc tSS_ijbc tSS_ijac.
// Relaxed: the occupied-virtual Lagrangian, with the pair symmetry w_ijab = w_jiba folding the reference's four terms into two,
//     L_ia = 2 sum_jbc w_ijbc (ab|jc) - 2 sum_jkb w_jkab (ji|kb) + [C_o^T (4 J[P_src] - 2 K[P_src]) C_v]_ia,   P_src = C P^(2) C^T.
// No array with three virtual indices is formed: the first term is the trace W1 of tf_mp4.hip.h over the occupied back-transformation of
// the AO-direct ladder of w (OV_ij[k][a] = sum_cd (kc|ad) w_ijcd, first term = 2 sum_j OV_ji[j][a]); the second is o GEMMs over the block
// (ji|kb); the third is one J/K build.  Then (A + B) z = -L with the singlet A + B of tf_cis.hip.h (rocSOLVER dpotrf / dpotrs, the
// caller), P_ia += z_ia / 2, P_ai += z_ia / 2.  Every reduction has one owner and a fixed order: bitwise repeatable, no atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace tfmp2dens {

// Amplitudes and the MP2 partials in one pass over g[i][a][j][b] = (ia|jb) (the loop and the reduction of tfmp3::mp3_amp_kernel):
//     tos[i][a][j][b] = tOS_ijab,   tss[i][a][j][b] = tSS_ijab                        (the operands of the unrelaxed GEMMs)
//     wov[i][a][j][b] = w_ijab  (the (ji|kb) GEMMs),   woo[i][j][a][b] = w_ijab  (the pair matrices of the ladder); both may be null
// D is summed as (e_i + e_j) - (e_a + e_b), the same bits for (ij, ab) and (ji, ba): with (ia|jb) = (jb|ia) to the last bit, as the
// transformation makes it, w_ijab = w_jiba to the last bit, which the stored-triangle ladder relies on (T_ji = T_ij^T).
__global__ void mp2dens_amp_kernel(const double *__restrict__ g, const double *__restrict__ eps, int n_frozen, int o, int v, int n_occ_total,
                                   double c_os, double c_ss, double *__restrict__ tos, double *__restrict__ tss, double *__restrict__ wov,
                                   double *__restrict__ woo, double *__restrict__ partial /* [gridDim.x][2] */)
{
#pragma clang fp contract(off)    // both images of an element round alike
    __shared__ double s_os[256], s_ss[256];
    const long long total = (long long)o * v * o * v;
    double os = 0.0, ss = 0.0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int j = (int)(r % o); r /= o;
        const int a = (int)(r % v);
        const int i = (int)(r / v);
        const double gij = g[e];
        const double gx = g[(((long long)i * v + b) * o + j) * v + a];
        const double D = (eps[n_frozen + i] + eps[n_frozen + j]) - (eps[n_occ_total + a] + eps[n_occ_total + b]);
        os += gij * gij / D;
        ss += gij * (gij - gx) / D;
        tos[e] = -2.0 * gij / D;
        tss[e] = (gij - gx) / D;
        if (wov) {
            const double w = (c_os * (2.0 * gij) + c_ss * (2.0 * (gij - gx))) / D;
            wov[e] = w;
            woo[(((long long)i * o + j) * v + a) * v + b] = w;
        }
    }
    s_os[threadIdx.x] = os; s_ss[threadIdx.x] = ss;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s_os[threadIdx.x] += s_os[threadIdx.x + s]; s_ss[threadIdx.x] += s_ss[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s_os[0]; partial[2 * blockIdx.x + 1] = s_ss[0]; }
}

// The Lagrangian, one thread per (i, a): the trace of the ladder's occupied back-transformation,
//     W1 = sum_k OV_ki[k][a],   OV_p[k][a] = A[p][k][a] (+ B[p'][a][k] when A, B hold the two images C_o^T Zh_p C_v and C_v^T Zh_p C_o of
//     the stored triangle's half: Z_ij = Zh_ij + Zh_ji^T; tfmp4::mp4_singles_kernel's W1), k ascending,
// then L = (2 W1 - 2 L2[ia]) + Lf[ia] in this order, L2 = sum_jkb w_jkab (ji|kb) and Lf the Fock response; rhs = -L (the right-hand side
// of the Z-vector equations, overwritten by their solution).
__global__ void mp2dens_lagrangian_kernel(const double *__restrict__ A, const double *__restrict__ B, int both_halves, const double *__restrict__ L2,
                                          const double *__restrict__ Lf, int o, int v, double *__restrict__ L, double *__restrict__ rhs)
{
    const long long ia = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ia >= (long long)o * v) return;
    const int i = (int)(ia / v), a = (int)(ia - (long long)i * v);
    double W1 = 0.0;
    for (int k = 0; k < o; ++k) {
        const long long ki = (long long)k * o + i, ik = (long long)i * o + k;
        double w1 = A[(ki * o + k) * v + a];
        if (both_halves) w1 += B[(ik * v + a) * o + k];
        W1 += w1;
    }
    const double l = (2.0 * W1 - 2.0 * L2[ia]) + Lf[ia];
    L[ia] = l;
    rhs[ia] = -l;
}

// P [N][N] in the MO basis from its blocks: Poo [o][o] in the occupied window [n_frozen, n_occ), Pvv [v][v] in the virtual window
// [n_occ, N), z [n_occ - n_frozen][v] / 2 in both occupied-virtual blocks (null: none), and -- with_reference -- the 2 of the
// Hartree-Fock determinant on the diagonal of every occupied orbital, the frozen ones included.  The two triangles of Poo and Pvv
// are averaged, so P is symmetric to the last bit.
__global__ void mp2dens_assemble_kernel(const double *__restrict__ Poo, const double *__restrict__ Pvv, const double *__restrict__ z, int with_reference,
                                        int N, int n_frozen, int n_occ, double *__restrict__ P)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)N * N) return;
    const int p = (int)(e / N), q = (int)(e - (long long)p * N);
    const int o = n_occ - n_frozen, v = N - n_occ;
    double x = 0.0;
    if (p < n_occ && q < n_occ) {
        if (p >= n_frozen && q >= n_frozen) {
            const int i = p - n_frozen, j = q - n_frozen;
            x = 0.5 * (Poo[(long long)i * o + j] + Poo[(long long)j * o + i]);
        }
        if (with_reference && p == q) x += 2.0;
    } else if (p >= n_occ && q >= n_occ) {
        const int a = p - n_occ, b = q - n_occ;
        x = 0.5 * (Pvv[(long long)a * v + b] + Pvv[(long long)b * v + a]);
    } else if (z) {
        const int i = (p < q ? p : q) - n_frozen, a = (p < q ? q : p) - n_occ;
        if (i >= 0) x = 0.5 * z[(long long)i * v + a];
    }
    P[e] = x;
}

// Natural orbitals: occ[k] = vals[n - 1 - k] and orb[mu][k] = V[mu][n - 1 - k], the eigenvalues in descending order
__global__ void natorb_reverse_kernel(const double *__restrict__ vals, const double *__restrict__ V, int n, double *__restrict__ occ, double *__restrict__ orb)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n * n) return;
    const int mu = (int)(e / n), k = (int)(e - (long long)mu * n);
    orb[e] = V[(long long)mu * n + (n - 1 - k)];
    if (mu == 0) occ[k] = vals[n - 1 - k];
}

}  // namespace tfmp2dens
