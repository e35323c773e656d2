// tf_mp4.hip.h -- restricted MP4(SDQ) and MP4(DQ) on the HBM-resident tensor (run_restricted_MP4, tuna_mp.py:1552-1685, without the
// triples).  Notation of tf_mp3.hip.h: occupied i, j, k, l (o orbitals), virtual a, b, c, d (v orbitals), D = e_i + e_j - e_a - e_b,
// t = (ia|jb) / D, t' = 2 [2 (ia|jb) - (ib|ja)] / D, L_pqrs = 2 (pq|rs) - (ps|rq), X[.] = MP3's operator (1/2 pp + 1/2 hh + ring).
//     doubles:     t2_ijab = (X[t]_ijab + X[t]_jiba) / D,                      E_D = sum t' X[t2]
//     singles:     u_ia = sum_kld t_klad L_kild - sum_kcd t_kicd L_adkc,        t1_ia = -u_ia / (e_i - e_a),
//                  S_ijab = sum_c t1_jc (ai|bc) - sum_k t1_kb (ai|kj),          E_S = sum t' S
//     quadruples:  the six products of t, t and (kc|ld) below,                  E_Q = sum t' Q
// Doubles: a second pass of the MP3 stages (ladder, hole-hole, ring, mp3_energy_kernel) on t2, written by mp4_t2_kernel in the operand
// layouts of mp3_amp_kernel.
// Singles: no integral with three virtual indices is formed.  The first ladder pass back-transforms every pair matrix with the occupied
// coefficients as well, OV_ij[k][a] = [C_o^T Z_ij C_v]_ka = sum_cd (kc|ad) t_ijcd, and with
//     W1_ia = sum_k OV_ki[k][a] = sum_kcd (kc|ad) t_kicd,      W2_ia = sum_k OV_ik[k][a] = sum_kcd (kc|ad) t_ikcd
// the (vv|ov) terms are  sum_kcd t_kicd L_adkc = 2 W1 - W2  and  sum_iab t'_ijab (ai|bc) = 4 W1_jc - 2 W2_jc  (t' = 4 t - 2 t^x).  With
// q[k][i][l][d] = (ki|ld), an o^3 v block of the AO->MO transformation, the rest is
//     u1_ia = sum_kld t_klad [2 q[k][i][l][d] - q[l][i][k][d]],      R_ia = sum_jld t'_jlad q[i][j][l][d]   (= sum_jlb' t'_ljb'a (b'l|ij))
//     E_S = sum_ia t1_ia (4 W1_ia - 2 W2_ia - R_ia).
// Quadruples (tuna_mp.py:1645-1650), GEMMs of the caller over tf_ccd.hip.h's operand layouts, all [(ov)][(ov)] unless noted:
//     Tn[(kc)][(jb)] = t_kjcb (= mp3_amp_kernel's tov)   Tx[(kc)][(jb)] = t_kjbc (= its tsw)   G = (kc|ld) (the block itself)
//     Gx[(ld)][(kc)] = (lc|kd)   Gw = 2 G - Gx = L[o,v,o,v]   Goo[(kl)][(cd)] = (kc|ld)
//     QA[(ij)][(ab)] = 1/2 (t Goo^T) t  -  F t  -  t_ij Fv^T      F[j][k] = Tn[j][(cld)] Gw[k][(cld)]^T,  Fv[b][c] = sum_k Tn_k[b][(ld)] Gw_k[c][(ld)]^T
//     QB[(ia)][(jb)] = Tn ((Tn - Tx) Gw)^T + 1/2 Tx (Tx G)^T         QC[(ja)][(ib)] = 1/2 Tx (Tx Gx)^T
//     E_Q = sum t'_ijab (QA[ij][ab] + QB[(ia)][(jb)] + QC[(ja)][(ib)])
// (F t lands on the (ji, ba) image of its term, which t' does not tell apart.)  Every reduction is per block, the blocks summed in block
// order by one thread: bitwise repeatable, no atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace tfmp4 {

// X[t]_ijab from the first pass's stages: the arguments of tfmp3::mp3_energy_kernel
__device__ __forceinline__ double mp4_x(const double *__restrict__ Y, int both_halves, const double *__restrict__ Xhh, const double *__restrict__ S13,
                                        const double *__restrict__ S2, int o, int v, int i, int j, int a, int b)
{
    const long long ijab = (((long long)i * o + j) * v + a) * v + b;
    double pp = Y[ijab];
    if (both_halves) pp += Y[(((long long)j * o + i) * v + b) * v + a];
    return pp + Xhh[ijab] + (S13[(((long long)i * v + a) * o + j) * v + b] - S2[(((long long)j * v + a) * o + i) * v + b]);
}

// The fused symmetrise-and-divide: t2 = (X_ijab + X_jiba) / D in the three operand layouts of the second pass (those of
// tfmp3::mp3_amp_kernel).  The two images are added as two complete sums: t2 is symmetric under (ij)(ab) to the last bit, which the
// stored-triangle ladder relies on (T_ji = T_ij^T).
__global__ void mp4_t2_kernel(const double *__restrict__ Y, int both_halves, const double *__restrict__ Xhh, const double *__restrict__ S13,
                              const double *__restrict__ S2, const double *__restrict__ eps, int n_frozen, int n_occ_total, int o, int v,
                              double *__restrict__ tov, double *__restrict__ too, double *__restrict__ tsw)
{
    const long long total = (long long)o * o * v * v;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int a = (int)(r % v); r /= v;
        const int j = (int)(r % o);
        const int i = (int)(r / o);
        const double X = mp4_x(Y, both_halves, Xhh, S13, S2, o, v, i, j, a, b) + mp4_x(Y, both_halves, Xhh, S13, S2, o, v, j, i, b, a);
        const double D = (eps[n_frozen + i] + eps[n_frozen + j]) - (eps[n_occ_total + a] + eps[n_occ_total + b]);   // (the same for (ji, ba))
        const double t2 = X / D;
        too[e] = t2;
        tov[(((long long)i * v + a) * o + j) * v + b] = t2;
        tsw[(((long long)j * v + a) * o + i) * v + b] = t2;
    }
}

// The quadruples' integral operands from (ia|jb) = g1[i][a][j][b] (the kernel of tfccd::cc_integral_operands_kernel, without H and Moo)
__global__ void mp4_integral_operands_kernel(const double *__restrict__ g1, int o, int v, double *__restrict__ Gx, double *__restrict__ Gw,
                                             double *__restrict__ Goo)
{
    const long long ov = (long long)o * v, total = ov * ov;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long kc = e / ov, jb = e - kc * ov;
        const int k = (int)(kc / v), c = (int)(kc - (long long)k * v);
        const int j = (int)(jb / v), b = (int)(jb - (long long)j * v);
        const double g = g1[e], gx = g1[(((long long)k * v + b) * o + j) * v + c];
        Gx[e] = gx;
        Gw[e] = 2.0 * g - gx;
        Goo[(((long long)k * o + j) * v + c) * v + b] = g;
    }
}

// The singles, one workgroup per (i, a):
//     u1 = sum_kld too[k][l][a][d] (2 q[k][i][l][d] - q[l][i][k][d]),   R = sum_jld tp[j][l][a][d] q[i][j][l][d]      (d fastest: coalesced)
//     W1 = sum_k OV_ki[k][a],  W2 = sum_k OV_ik[k][a],   OV_p[k][a] = A[p][k][a] (+ B[p'][a][k] when A, B hold the two back-transformed
//     images C_o^T Zh_p C_v and C_v^T Zh_p C_o of the stored triangle's half: Z_ij = Zh_ij + Zh_ji^T)
//     t1 = -(u1 - (2 W1 - W2)) / (e_i - e_a),   partial[(ia)] = t1 (4 W1 - 2 W2 - R)
__global__ void mp4_singles_kernel(const double *__restrict__ too, const double *__restrict__ tp, const double *__restrict__ q,
                                   const double *__restrict__ A, const double *__restrict__ B, int both_halves, const double *__restrict__ eps,
                                   int n_frozen, int n_occ_total, int o, int v, double *__restrict__ t1, double *__restrict__ partial)
{
    __shared__ double s_u[256], s_r[256];
    const int i = blockIdx.x / v, a = blockIdx.x - i * v;
    const long long total = (long long)o * o * v;
    double u1 = 0.0, R = 0.0;
    for (long long e = threadIdx.x; e < total; e += blockDim.x) {
        long long r = e;
        const int d = (int)(r % v); r /= v;
        const int l = (int)(r % o);
        const int k = (int)(r / o);
        const long long klad = (((long long)k * o + l) * v + a) * v + d;
        const double qk = q[(((long long)k * o + i) * o + l) * v + d], ql = q[(((long long)l * o + i) * o + k) * v + d];
        u1 += too[klad] * (2.0 * qk - ql);
        R += tp[klad] * q[(((long long)i * o + k) * o + l) * v + d];
    }
    s_u[threadIdx.x] = u1; s_r[threadIdx.x] = R;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s_u[threadIdx.x] += s_u[threadIdx.x + s]; s_r[threadIdx.x] += s_r[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double W1 = 0.0, W2 = 0.0;
        for (int k = 0; k < o; ++k) {
            const long long ki = (long long)k * o + i, ik = (long long)i * o + k;
            double w1 = A[(ki * o + k) * v + a], w2 = A[(ik * o + k) * v + a];
            if (both_halves) { w1 += B[(ik * v + a) * o + k]; w2 += B[(ki * v + a) * o + k]; }
            W1 += w1; W2 += w2;
        }
        const double u = s_u[0] - (2.0 * W1 - W2);
        const double t = -u / (eps[n_frozen + i] - eps[n_occ_total + a]);
        t1[blockIdx.x] = t;
        partial[blockIdx.x] = t * (4.0 * W1 - 2.0 * W2 - s_r[0]);
    }
}

// The component-energy reduction: partial[block] = sum t'_ijab (QA[ij][ab] + QB[(ia)][(jb)] + QC[(ja)][(ib)]) over the block's share of
// (ijab), in the order of a fixed grid (tfccd::cc_sum_partials_kernel adds the blocks in block order)
__global__ void mp4_energy_kernel(const double *__restrict__ tp, const double *__restrict__ QA, const double *__restrict__ QB,
                                  const double *__restrict__ QC, int o, int v, double *__restrict__ partial)
{
    __shared__ double s_e[256];
    const long long total = (long long)o * o * v * v;
    double en = 0.0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int a = (int)(r % v); r /= v;
        const int j = (int)(r % o);
        const int i = (int)(r / o);
        en += tp[e] * (QA[e] + QB[(((long long)i * v + a) * o + j) * v + b] + QC[(((long long)j * v + a) * o + i) * v + b]);
    }
    s_e[threadIdx.x] = en;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_e[threadIdx.x] += s_e[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s_e[0];
}

}  // namespace tfmp4
