// tf_ccd.hip.h -- restricted LCCD and CCD iterated on the HBM-resident tensor (run_restricted_LCCD_iteration, tuna_cc.py:830-864;
// run_restricted_CCD_iteration, tuna_cc.py:915-960).  Notation of tf_mp3.hip.h: occupied i, j, k, l (o orbitals), virtual a, b, c, d
// (v orbitals), D = e_i + e_j - e_a - e_b.  One step:
//     R_ijab = 1/2 (ia|jb) + 1/2 sum_kl W_ijkl t_klab + 1/2 sum_cd (ac|bd) t_ijcd + sum_c F_ca t_ijcb - sum_k F_ik t_kjab
//            + sum_kc W_icak (2 t_kjcb - t_kjbc) - sum_kc W_ciak t_kjcb - sum_kc W_cibk t_kjac,      t_ijab <- (R_ijab + R_jiba) / D
// LCCD: F = 0, W_ijkl = (ik|jl), W_icak = (ia|kc), W_ciak = (ik|ac).  CCD (w_cdkl = 2 (ck|dl) - (dk|cl)):
//     F_ik = sum_lcd w_cdkl t_ilcd,   F_ca = -sum_kld w_cdkl t_klad,   W_ijkl = (ik|jl) + sum_cd (ck|dl) t_ijcd,
//     W_icak = (ia|kc) - 1/2 sum_ld (dl|ck) t_ilda + 1/2 sum_ld w_dclk t_ilad,   W_ciak = (ik|ac) - 1/2 sum_ld (cl|dk) t_ilda
// Everything but the particle-particle ladder is a GEMM over these operands (the caller, tf_corr_host.hip.h), all [(ov)][(ov)] unless noted:
//     G [(ia)][(kc)] = (ia|kc) (the block itself)   Gx[(ld)][(kc)] = (lc|kd)   Gw = 2 G - Gx   H[(ia)][(kc)] = (ik|ac)
//     Goo[(kl)][(cd)] = (kc|ld)   Moo[(ij)][(kl)] = (ik|jl)
//     Tn[(kc)][(jb)] = t_kjcb   Tx[(kc)][(jb)] = t_kjbc   Tm = 2 Tn - Tx                    (from t[i][j][a][b] every step)
//     A1 = W_icak as [(ia)][(kc)] = G + 1/2 Tn Gw - 1/2 Tx G,   A2 = W_ciak as [(ia)][(kc)] = H - 1/2 Tx Gx
//     S1[(ia)][(jb)] = A1 Tm - A2 Tn,   S2[(ib)][(ja)] = A2 Tx,   X[(ij)][(ab)] = 1/2 W t + F_ca^T t_ij - F_ik t
// The ladder is tf_mp3.hip.h's, on the pair matrices of the current amplitudes.  Every reduction here is per block, the blocks summed
// in block order by one thread: bitwise repeatable, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include "tf_cc_diis.h"   // the host side of the DIIS: diis_solve, DiisHistory

namespace tfccd {

// Guess amplitudes t[i][j][a][b] = (ia|jb) / D and the MP2 partials, in the loop and the reduction of tfmp3::mp3_amp_kernel (so that
// the MP2 energy is bit for bit that of tf_mp2_rhf): partial[block][2] = {opposite spin, same spin}
__global__ void cc_guess_kernel(const double *__restrict__ g, const double *__restrict__ eps, int n_frozen, int o, int v, int n_occ_total,
                                double *__restrict__ t, double *__restrict__ partial)
{
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
        const double D = eps[n_frozen + i] + eps[n_frozen + j] - eps[n_occ_total + a] - eps[n_occ_total + b];
        os += gij * gij / D;
        ss += gij * (gij - gx) / D;
        t[(((long long)i * o + j) * v + a) * v + b] = gij / D;
    }
    s_os[threadIdx.x] = os; s_ss[threadIdx.x] = ss;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s_os[threadIdx.x] += s_os[threadIdx.x + s]; s_ss[threadIdx.x] += s_ss[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s_os[0]; partial[2 * blockIdx.x + 1] = s_ss[0]; }
}

// The integral operands, once per calculation, from (ia|jb) = g1[i][a][j][b], (ab|ij) = g2[a][b][i][j], (ki|lj) = g3[k][i][l][j].
// Gx, Gw and Goo are CCD's (NULL for LCCD).
__global__ void cc_integral_operands_kernel(const double *__restrict__ g1, const double *__restrict__ g2, const double *__restrict__ g3, int o, int v,
                                            double *__restrict__ H, double *__restrict__ Moo, double *__restrict__ Gx, double *__restrict__ Gw,
                                            double *__restrict__ Goo)
{
    const long long ov = (long long)o * v, n2 = ov * ov, n4 = (long long)o * o * o * o, total = n2 > n4 ? n2 : n4;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        if (e < n2) {
            const long long kc = e / ov, jb = e - kc * ov;
            const int k = (int)(kc / v), c = (int)(kc - (long long)k * v);
            const int j = (int)(jb / v), b = (int)(jb - (long long)j * v);
            H[e] = g2[(((long long)c * v + b) * o + k) * o + j];      // (kj|cb)
            if (Gx) {
                const double g = g1[e], gx = g1[(((long long)k * v + b) * o + j) * v + c];
                Gx[e] = gx;
                Gw[e] = 2.0 * g - gx;
                Goo[(((long long)k * o + j) * v + c) * v + b] = g;
            }
        }
        if (e < n4) {
            long long r = e;
            const int l = (int)(r % o); r /= o;
            const int k = (int)(r % o); r /= o;
            const int j = (int)(r % o);
            const int i = (int)(r / o);
            Moo[e] = g3[(((long long)i * o + k) * o + j) * o + l];    // Moo[i j][k l] = (ik|jl)
        }
    }
}

// The amplitude operands of a step from t[i][j][a][b]
__global__ void cc_amplitude_operands_kernel(const double *__restrict__ t, int o, int v, double *__restrict__ Tn, double *__restrict__ Tx,
                                             double *__restrict__ Tm)
{
    const long long total = (long long)o * v * o * v;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int j = (int)(r % o); r /= o;
        const int c = (int)(r % v);
        const int k = (int)(r / v);
        const long long kj = ((long long)k * o + j) * v;
        const double tn = t[(kj + c) * v + b], tx = t[(kj + b) * v + c];
        Tn[e] = tn;
        Tx[e] = tx;
        Tm[e] = 2.0 * tn - tx;
    }
}

// R_ijab before the (ji, ba) image, in one fixed order of its terms.  Y = the back-transformed ladder 1/2 C_v^T Zh C_v [ij][a][b]; with
// both_halves (the packed layout) it holds the stored triangle's half and the ladder is Y[ij][a][b] + Y[ji][b][a].
__device__ __forceinline__ double cc_residual(const double *__restrict__ g1, const double *__restrict__ Y, int both_halves,
                                              const double *__restrict__ X, const double *__restrict__ S1, const double *__restrict__ S2, int o,
                                              int v, int i, int j, int a, int b)
{
    const long long ijab = (((long long)i * o + j) * v + a) * v + b;
    const long long iajb = (((long long)i * v + a) * o + j) * v + b;
    double pp = Y[ijab];
    if (both_halves) pp += Y[(((long long)j * o + i) * v + b) * v + a];
    return 0.5 * g1[iajb] + X[ijab] + pp + S1[iajb] - S2[(((long long)i * v + b) * o + j) * v + a];
}

// The fused update, one pass over [i][j][a][b]: t_new = (R_ijab + R_jiba) / D, dt = t_new - t, and partial[block][2] =
// {sum [2 (ia|jb) - (ib|ja)] t_new, sum dt^2} over the block's share, summed in the order of a fixed grid.  The two images are added as
// two complete sums: t_new is symmetric under (ij)(ab) to the last bit.
__global__ void cc_update_kernel(const double *__restrict__ g1, const double *__restrict__ eps, int n_frozen, int n_occ_total, int o, int v,
                                 const double *__restrict__ t, const double *__restrict__ Y, int both_halves, const double *__restrict__ X,
                                 const double *__restrict__ S1, const double *__restrict__ S2, double *__restrict__ t_new, double *__restrict__ dt,
                                 double *__restrict__ partial)
{
    __shared__ double s_e[256], s_d[256];
    const long long total = (long long)o * o * v * v;
    double en = 0.0, d2 = 0.0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int a = (int)(r % v); r /= v;
        const int j = (int)(r % o);
        const int i = (int)(r / o);
        const double R = cc_residual(g1, Y, both_halves, X, S1, S2, o, v, i, j, a, b) + cc_residual(g1, Y, both_halves, X, S1, S2, o, v, j, i, b, a);
        const double D = (eps[n_frozen + i] + eps[n_frozen + j]) - (eps[n_occ_total + a] + eps[n_occ_total + b]);   // (the same for (ji, ba))
        const double tn = R / D, d = tn - t[e];
        t_new[e] = tn;
        dt[e] = d;
        en += (2.0 * g1[(((long long)i * v + a) * o + j) * v + b] - g1[(((long long)i * v + b) * o + j) * v + a]) * tn;
        d2 += d * d;
    }
    s_e[threadIdx.x] = en; s_d[threadIdx.x] = d2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s_e[threadIdx.x] += s_e[threadIdx.x + s]; s_d[threadIdx.x] += s_d[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s_e[0]; partial[2 * blockIdx.x + 1] = s_d[0]; }
}

// out[q] = sum over the blocks, in block order, of partial[block][q] (q < nq): one thread per sum
__global__ void cc_sum_partials_kernel(const double *__restrict__ partial, int nblk, int nq, double *__restrict__ out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partial[(size_t)b * nq + q];
    out[q] = s;
}

// DIIS: the dot products of the newest error vector with the n vectors of the history, hist[slot[m]] . hist[slot[newest]]; grid
// (blocks, n), partial[block][m]
__global__ void cc_diis_dots_kernel(const double *__restrict__ hist, long long stride, const int *__restrict__ slot, int n, int newest, long long total,
                                    double *__restrict__ partial)
{
    __shared__ double s_d[256];
    const int m = blockIdx.y;
    const double *__restrict__ x = hist + (size_t)slot[m] * stride, *__restrict__ y = hist + (size_t)slot[newest] * stride;
    double d = 0.0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) d += x[e] * y[e];
    s_d[threadIdx.x] = d;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_d[threadIdx.x] += s_d[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)blockIdx.x * n + m] = s_d[0];
}

// The amplitudes of the next step: x = sum_m coef[m] hist[slot[m]] (n > 0: the DIIS extrapolation, in the order of the history) or
// t_new (n == 0), then t <- damping t + (1 - damping) x
__global__ void cc_mix_kernel(double *__restrict__ t, const double *__restrict__ t_new, const double *__restrict__ hist, long long stride,
                              const int *__restrict__ slot, const double *__restrict__ coef, int n, double damping, long long total)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        double x;
        if (n > 0) {
            x = 0.0;
            for (int m = 0; m < n; ++m) x += coef[m] * hist[(size_t)slot[m] * stride + e];
        } else {
            x = t_new[e];
        }
        t[e] = damping * t[e] + (1.0 - damping) * x;
    }
}

}  // namespace tfccd
