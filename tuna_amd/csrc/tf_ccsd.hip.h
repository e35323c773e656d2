// tf_ccsd.hip.h -- restricted LCCSD, QCISD and CCSD iterated on the HBM-resident tensor (run_restricted_LCCSD_iteration,
// tuna_cc.py:1020-1063; run_restricted_QCISD_iteration, :1503-1557; run_restricted_CCSD_iteration, :1638-1718).  Notation of
// tf_ccd.hip.h; t1[i][a], D_ia = e_i - e_a, th = t2 (LCCSD, QCISD) or t2 + t1 t1 (CCSD), b_i = C_v t_i, w_kcld = 2 (kc|ld) - (kd|lc).
// Nothing here or in the caller has three virtual indices.  The ladder runs once per step on the dressed pair matrices
//     T_ij = C_v th_ij C_v^T + c_i b_j^T + b_i c_j^T,      Z_ij[mu][nu] = sum (mu la|nu si) T_ij[la][si],
// whose back-transformation gives  Y_ij = 1/2 C_v^T Z_ij C_v = 1/2 sum_cd (ac|bd) th_ijcd + 1/2 [(ia|b_j b) + (b_i a|jb)]   (the ladder and,
// after the (ji, ba) image, sum_c (ia|cb) t_jc with its image)  and  O_ij[k][a] = c_k^T Z_ij c_a = sum_cd (kc|ad) th_ijcd + (ki|a b_j) +
// (k b_i|aj).  One step (terms in this order in the kernels):
//   singles  s_ia = sum_k [2 O_ki[k][a] - O_ik[k][a]] - sum_c t_ic G2e_ca - sum_klc [2 (ik|lc) - (il|kc)] th_klac
//                   (QCISD, CCSD) + sum_c F_ca t_ic - sum_k F_ik t_ka + sum_kc F_kc (2 t_kica - t_ikca)   (CCSD) + sum_k t_ka sum_c F_kc t_ic
//            The O sums hold sum_kcd [2 (ac|kd) - (ad|kc)] th_ikcd + sum_kc [2 (ia|kc) - (ik|ac)] t_kc + sum_c t_ic G2e_ca with
//            G2e_ca = sum_k 2 (kk|ca) - (kc|ka), which is why G2e leaves again.   t_ia <- s_ia / D_ia
//   doubles  R_ijab = tf_ccd.hip.h's R_ijab (ladder = Y above; W_ijkl, F multiply th where the reference has t2 + t1 t1)
//                   - sum_k (ia|jk) t_kb   (CCSD) - sum_k t_ka O_ij[k][b]
//            LCCSD: F = 0 and bare W.  QCISD: CCD's F_ik, F_ca, W_ijkl, W_icak, W_ciak.  CCSD: F_ik, F_ca on th plus the oo and vv blocks of
//            M = 2 J - K of the density C_o t1 C_v^T (L_ik, L_ca);  W_ijkl = (ik|jl) + sum_cd (kc|ld) th_ijcd + P_ijkl + P_jilk,
//            P_ijkl = sum_c t_ic (kc|jl);  W_icak = (l_i x_a|kc) + CCD's t2 terms, W_ciak = (l_i k|x_a c) + CCD's t2 term, l_i = c_i + b_i,
//            x_a = c_a - sum_k c_k t_ka (two AO->MO transformations with dressed coefficients per step).  The last CCSD term is the t1 part of
//            W_cdab together with -(ik|cb) t_ka t_jc and -(ia|ck) t_jc t_kb.
//   energy   connected = sum [2 (ia|jb) - (ib|ja)] t_ijab, disconnected (CCSD) = sum [2 (ia|jb) - (ib|ja)] t_ia t_jb, both on the new amplitudes
// t1 lies directly behind t2 in the amplitude buffers (t, t_new, dt and every DIIS slot), so tf_ccd.hip.h's DIIS and mixing kernels run
// over o^2 v^2 + ov elements.  Reductions as in tf_ccd.hip.h: per block, blocks summed in block order, no atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace tfccsd {

// The rank-one dressing of a batch of pair matrices: Tm[p][mu][nu] += Co[mu][i] Bo[nu][j] + Bo[mu][i] Co[nu][j], (i, j) the pair p0 + p
// (transposed: the batch holds T^T, the pair is read as (j, i)).  nu fastest: coalesced over the matrices' rows.
__global__ void ccsd_dress_pairs_kernel(double *__restrict__ Tm, int N, int nb, int p0, int o, const double *__restrict__ Co,
                                        const double *__restrict__ Bo, int transposed)
{
    const long long nn = (long long)N * N, total = nn * nb;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(e / nn);
        const long long mn = e - (long long)p * nn;
        const int mu = (int)(mn / N), nu = (int)(mn - (long long)mu * N);
        int i = (p0 + p) / o, j = (p0 + p) - i * o;
        if (transposed) { const int s = i; i = j; j = s; }
        Tm[e] += Co[(long long)mu * o + i] * Bo[(long long)nu * o + j] + Bo[(long long)mu * o + i] * Co[(long long)nu * o + j];
    }
}

// th[i][j][a][b] = t2[i][j][a][b] + t1[i][a] t1[j][b]
__global__ void ccsd_tau_kernel(const double *__restrict__ t2, const double *__restrict__ t1, int o, int v, double *__restrict__ th)
{
    const long long total = (long long)o * o * v * v;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int a = (int)(r % v); r /= v;
        const int j = (int)(r % o);
        const int i = (int)(r / o);
        th[e] = t2[e] + t1[(long long)i * v + a] * t1[(long long)j * v + b];
    }
}

// G2e[c][a] = sum_k 2 (kk|ca) - (kc|ka) from H[(ia)][(kc)] = (ik|ac) and g1[i][a][j][b] = (ia|jb); once per calculation
__global__ void ccsd_g2e_kernel(const double *__restrict__ H, const double *__restrict__ g1, int o, int v, double *__restrict__ G2e)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= v * v) return;
    const int c = e / v, a = e - c * v;
    const long long ov = (long long)o * v;
    double s = 0.0;
    for (int k = 0; k < o; ++k) {
        const long long kc = (long long)k * v + c, ka = (long long)k * v + a;
        s += 2.0 * H[kc * ov + ka] - g1[kc * ov + ka];
    }
    G2e[e] = s;
}

// A2[(ia)][(kc)] = q[a][c][i][k], the (ab|ij)-ordered block of a sliced transformation as an [(ov)][(ov)] operand
__global__ void ccsd_vvoo_operand_kernel(const double *__restrict__ q, int o, int v, double *__restrict__ A2)
{
    const long long ov = (long long)o * v, total = ov * ov;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long ia = e / ov, kc = e - ia * ov;
        const int i = (int)(ia / v), a = (int)(ia - (long long)i * v);
        const int k = (int)(kc / v), c = (int)(kc - (long long)k * v);
        A2[e] = q[(((long long)a * v + c) * o + i) * o + k];
    }
}

// F_kc = sum_ld Gw[(kc)][(ld)] t1[(ld)]: one workgroup per (kc), a fixed tree
__global__ void ccsd_fkc_kernel(const double *__restrict__ Gw, const double *__restrict__ t1, int ov, double *__restrict__ Fkc)
{
    __shared__ double s_f[256];
    const double *__restrict__ row = Gw + (long long)blockIdx.x * ov;
    double f = 0.0;
    for (int e = threadIdx.x; e < ov; e += blockDim.x) f += row[e] * t1[e];
    s_f[threadIdx.x] = f;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_f[threadIdx.x] += s_f[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) Fkc[blockIdx.x] = s_f[0];
}

// W[(ij)][(kl)] += P_ijkl + P_jilk, P_ijkl = sum_c t1[i][c] q[j][l][k][c]   (q[i][k][j][a] = (ik|ja))
__global__ void ccsd_woo_dress_kernel(const double *__restrict__ q, const double *__restrict__ t1, int o, int v, double *__restrict__ W)
{
    const int total = o * o * o * o;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int r = e;
    const int l = r % o; r /= o;
    const int k = r % o; r /= o;
    const int j = r % o;
    const int i = r / o;
    const double *__restrict__ q1 = q + (((long long)j * o + l) * o + k) * v, *__restrict__ q2 = q + (((long long)i * o + k) * o + l) * v;
    double p1 = 0.0, p2 = 0.0;
    for (int c = 0; c < v; ++c) { p1 += t1[(long long)i * v + c] * q1[c]; p2 += t1[(long long)j * v + c] * q2[c]; }
    W[e] += p1 + p2;
}

// M = 2 J - K, in place of J
__global__ void ccsd_m_kernel(double *__restrict__ J, const double *__restrict__ K, long long total)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) J[e] = 2.0 * J[e] - K[e];
}

// O_ij[k][a] from the two back-transformed images of the ladder stage (tf_mp4.hip.h's convention): A[(ij)][k][a] and, with both_halves,
// + B[(ji)][a][k]
__device__ __forceinline__ double ccsd_ov_block(const double *__restrict__ A, const double *__restrict__ B, int both_halves, int o, int v, int i, int j,
                                                int k, int a)
{
    double x = A[(((long long)i * o + j) * o + k) * v + a];
    if (both_halves) x += B[(((long long)j * o + i) * v + a) * o + k];
    return x;
}

// The fused singles update, one workgroup per (i, a); level 0 LCCSD, 1 QCISD, 2 CCSD.  th = the amplitudes of the ladder, q = (ik|ja) as
// q[i][k][j][a].  Writes t1_new, dt1 and partial[(ia)] = dt1^2.
__global__ void ccsd_singles_kernel(int level, const double *__restrict__ t2, const double *__restrict__ th, const double *__restrict__ t1,
                                    const double *__restrict__ q, const double *__restrict__ OA, const double *__restrict__ OB, int both_halves,
                                    const double *__restrict__ G2e, const double *__restrict__ Fik, const double *__restrict__ Fca,
                                    const double *__restrict__ Fkc, const double *__restrict__ eps, int n_frozen, int n_occ_total, int o, int v,
                                    double *__restrict__ t1_new, double *__restrict__ dt1, double *__restrict__ partial)
{
    __shared__ double s_u[256], s_f[256];
    const int i = blockIdx.x / v, a = blockIdx.x - i * v;
    const long long total = (long long)o * o * v;
    double u = 0.0, f = 0.0;
    for (long long e = threadIdx.x; e < total; e += blockDim.x) {
        long long r = e;
        const int c = (int)(r % v); r /= v;
        const int l = (int)(r % o);
        const int k = (int)(r / o);
        u += (2.0 * q[(((long long)i * o + k) * o + l) * v + c] - q[(((long long)i * o + l) * o + k) * v + c]) * th[(((long long)k * o + l) * v + a) * v + c];
    }
    if (level >= 1) {
        const long long okc = (long long)o * v;
        for (long long e = threadIdx.x; e < okc; e += blockDim.x) {
            const int k = (int)(e / v), c = (int)(e - (long long)k * v);
            f += Fkc[e] * (2.0 * t2[(((long long)k * o + i) * v + c) * v + a] - t2[(((long long)i * o + k) * v + c) * v + a]);
        }
    }
    s_u[threadIdx.x] = u; s_f[threadIdx.x] = f;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s_u[threadIdx.x] += s_u[threadIdx.x + s]; s_f[threadIdx.x] += s_f[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double W1 = 0.0, W2 = 0.0, ge = 0.0;
        for (int k = 0; k < o; ++k) {
            W1 += ccsd_ov_block(OA, OB, both_halves, o, v, k, i, k, a);
            W2 += ccsd_ov_block(OA, OB, both_halves, o, v, i, k, k, a);
        }
        for (int c = 0; c < v; ++c) ge += t1[(long long)i * v + c] * G2e[(long long)c * v + a];
        double s = (2.0 * W1 - W2) - ge - s_u[0];
        if (level >= 1) {
            double fc = 0.0, fi = 0.0;
            for (int c = 0; c < v; ++c) fc += Fca[(long long)c * v + a] * t1[(long long)i * v + c];
            for (int k = 0; k < o; ++k) fi += Fik[(long long)i * o + k] * t1[(long long)k * v + a];
            s += fc - fi + s_f[0];
            if (level >= 2) {
                double x = 0.0;
                for (int k = 0; k < o; ++k) {
                    double y = 0.0;
                    for (int c = 0; c < v; ++c) y += Fkc[(long long)k * v + c] * t1[(long long)i * v + c];
                    x += t1[(long long)k * v + a] * y;
                }
                s += x;
            }
        }
        const double tn = s / (eps[n_frozen + i] - eps[n_occ_total + a]), d = tn - t1[blockIdx.x];
        t1_new[blockIdx.x] = tn;
        dt1[blockIdx.x] = d;
        partial[blockIdx.x] = d * d;
    }
}

// R_ijab before the (ji, ba) image: tfccd::cc_residual, then the singles' terms in a fixed order
__device__ __forceinline__ double ccsd_residual(int level, const double *__restrict__ g1, const double *__restrict__ Y, int both_halves,
                                                const double *__restrict__ X, const double *__restrict__ S1, const double *__restrict__ S2,
                                                const double *__restrict__ q, const double *__restrict__ t1, const double *__restrict__ OA,
                                                const double *__restrict__ OB, int o, int v, int i, int j, int a, int b)
{
    double R = tfccd::cc_residual(g1, Y, both_halves, X, S1, S2, o, v, i, j, a, b);
    double x = 0.0;
    for (int k = 0; k < o; ++k) x += q[(((long long)j * o + k) * o + i) * v + a] * t1[(long long)k * v + b];      // (jk|ia) t_kb
    R -= x;
    if (level >= 2) {
        double y = 0.0;
        for (int k = 0; k < o; ++k) y += t1[(long long)k * v + a] * ccsd_ov_block(OA, OB, both_halves, o, v, i, j, k, b);
        R -= y;
    }
    return R;
}

// The fused doubles update: tfccd::cc_update_kernel with ccsd_residual.  partial[block][2] = {connected energy, sum dt2^2}
__global__ void ccsd_update_kernel(int level, const double *__restrict__ g1, const double *__restrict__ eps, int n_frozen, int n_occ_total, int o,
                                   int v, const double *__restrict__ t, const double *__restrict__ Y, int both_halves, const double *__restrict__ X,
                                   const double *__restrict__ S1, const double *__restrict__ S2, const double *__restrict__ q,
                                   const double *__restrict__ t1, const double *__restrict__ OA, const double *__restrict__ OB,
                                   double *__restrict__ t_new, double *__restrict__ dt, double *__restrict__ partial)
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
        const double R = ccsd_residual(level, g1, Y, both_halves, X, S1, S2, q, t1, OA, OB, o, v, i, j, a, b) +
                         ccsd_residual(level, g1, Y, both_halves, X, S1, S2, q, t1, OA, OB, o, v, j, i, b, a);
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

// partial[block] = sum [2 (ia|jb) - (ib|ja)] t1[i][a] t1[j][b] over the block's share of (iajb): the disconnected energy
__global__ void ccsd_disconnected_kernel(const double *__restrict__ g1, const double *__restrict__ t1, int o, int v, double *__restrict__ partial)
{
    __shared__ double s_e[256];
    const long long total = (long long)o * v * o * v;
    double en = 0.0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int j = (int)(r % o); r /= o;
        const int a = (int)(r % v);
        const int i = (int)(r / v);
        en += (2.0 * g1[e] - g1[(((long long)i * v + b) * o + j) * v + a]) * t1[(long long)i * v + a] * t1[(long long)j * v + b];
    }
    s_e[threadIdx.x] = en;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_e[threadIdx.x] += s_e[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s_e[0];
}

}  // namespace tfccsd
