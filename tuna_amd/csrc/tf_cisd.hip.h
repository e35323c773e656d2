// tf_cisd.hip.h -- CIS(D): the perturbative doubles correction of Head-Gordon, Rico, Oumi and Lee (Chem. Phys. Lett. 219, 21 (1994)) to
// one closed-shell CIS or TDHF state (calculate_restricted_doubles_correction, tuna_ci.py:1874-1982), without any block with three
// virtual indices.  Notation of tf_mp3.hip.h and tf_cis.hip.h: occupied i, j, k (o orbitals), virtual a, b, c (v orbitals), compound
// index (ia) = i v + a, D_ijab = e_i + e_j - e_a - e_b, g = (ia|jb) [i][a][j][b], t = g / D.  The state: b_ia (normalised), energy w.
//
// Direct part.  With the dressed occupied orbitals Ct_o[:, i] = sum_c C_v[:, c] b_ic, the half-dressed block
//     M[i][a][j][b] = (i~ a|j b) - sum_k b_ka (ki|jb)
// holds all four of the reference's p_1, p_2, h_1, h_2:  u_S[ijab] = M[iajb] + M[jbia],  u_T[ijab] = M[iajb] - M[jbia].  With
// s = 1 / (D_ijab + w):
//     singlet: E_direct = sum s u_S[ijab] (u_S[ijab] - 1/2 u_S[jiab])
//     triplet: E_direct = 1/2 sum s (u_S[ijab]^2 - u_S[ijab] u_S[jiab] + u_T[ijab]^2)
//   * direct_kernel makes that sum in one pass over M.  A workgroup owns one pair (i, j) and one 16 x 16 tile of (a, b).  Of the four
//     elements of a term, M[iajb] and M[jaib] run along b, as the lanes of the second phase do, and are read straight into registers;
//     M[jbia] and M[ibja] run along a: they are read with a as the lane index into padded LDS tiles and picked up transposed (as
//     tfcis::assemble_kernel gathers its transposed operands).  Every global read is a run of up to 16 consecutive doubles, one 128-byte
//     line.  The 256 terms of a tile are added in a fixed tree, the tile's sum and its smallest |D + w| go to the block's own slots, and
//     the host adds the slots in block order: no atomics, two calls give the same bits.
//
// Indirect part.  L = 2 (jb|kc) - (jc|kb) and tt = 2 t_ikac - t_ikca, both [(jb)][(kc)] and symmetric; operands_kernel writes t, tt and
// L in one pass over g and eps with the same tiling (g[ibja] is the transposed read).  State-independent, by one GEMM each:
//     Goo_ij = sum_kbc L_jkbc t_ikbc  (rows i and j of t and L, o x o v^2 each),   Gvv_ba = sum_jkc L_jkbc t_jkac  (columns, o^2 v x v)
// Per state x = L b, y = tt x (singlet) or x = (2 g - L) b, y = (2 t - tt) x (triplet: (jc|kb) = 2 g - L and t_ikca = 2 t - tt), and
//     E_indirect = sum_ia b_ia y_ia - sum_ija b_ia b_ja Goo_ij - sum_iab b_ia b_ib Gvv_ba
// whose three sums of o v, o^2 v and o v^2 terms are made on the host in a fixed order.
//
// Work space of the driver (tf_cis_d_rhf, tf_excited_host.hip.h): 5 arrays of o^2 v^2 values -- g, t, tt, L and M -- plus, while a block
// is being transformed on the packed and tiles layouts, the 2 halves mo_transform_device adds up; (ki|jb) is o^3 v.  Nothing of size
// o v^3 or v^4 exists anywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace tfcisd {

#define TFD_T 16                  // tile edge: 16 doubles are one 128-byte line
#define TFD_P (TFD_T + 1)         // padded row of an LDS tile

// blocks of a pass over [i][a][j][b] in tiles of one (i, j) and TFD_T x TFD_T of (a, b)
inline long long tile_blocks(int o, int v)
{
    const long long nt = (v + TFD_T - 1) / TFD_T;
    return (long long)o * o * nt * nt;
}

// block -> pair (i, j) and the tile origin (a0, b0); the b tiles run fastest
__device__ __forceinline__ void tile_of_block(int o, int v, int &i, int &j, int &a0, int &b0)
{
    const int nt = (v + TFD_T - 1) / TFD_T;
    long long blk = blockIdx.x;
    b0 = (int)(blk % nt) * TFD_T; blk /= nt;
    a0 = (int)(blk % nt) * TFD_T; blk /= nt;
    j = (int)(blk % o);
    i = (int)(blk / o);
}

// t = g / D, tt = (2 g[iajb] - g[ibja]) / D, L = 2 g[iajb] - g[ibja], all [i][a][j][b]: block (16, 16), grid tile_blocks(o, v)
__global__ __launch_bounds__(256) void operands_kernel(const double *__restrict__ g, const double *__restrict__ eps, int n_frozen, int n_occ, int o,
                                                       int v, double *__restrict__ t, double *__restrict__ tt, double *__restrict__ L)
{
    __shared__ double sX[TFD_T][TFD_P];                       // [b - b0][a - a0] = g[i][b][j][a]
    int i, j, a0, b0;
    tile_of_block(o, v, i, j, a0, b0);
    const long long dim = (long long)o * v;
    const int tx = threadIdx.x, ty = threadIdx.y;
    {
        const int a = a0 + tx, b = b0 + ty;                   // lanes along a
        if (a < v && b < v) sX[ty][tx] = g[((long long)i * v + b) * dim + (long long)j * v + a];
    }
    __syncthreads();
    const int a = a0 + ty, b = b0 + tx;                       // lanes along b
    if (a >= v || b >= v) return;
    const long long e = ((long long)i * v + a) * dim + (long long)j * v + b;
    const double G = g[e], X = sX[tx][ty];
    const double D = (eps[n_frozen + i] + eps[n_frozen + j]) - (eps[n_occ + a] + eps[n_occ + b]);
    const double l = 2.0 * G - X;
    t[e] = G / D;
    tt[e] = l / D;
    L[e] = l;
}

// One state's direct part: part[block] = the tile's sum, pmin[block] = its smallest |D + w| (INFINITY for a tile without elements, which
// does not occur).  block (16, 16), grid tile_blocks(o, v)
__global__ __launch_bounds__(256) void direct_kernel(const double *__restrict__ M, const double *__restrict__ eps, int n_frozen, int n_occ, int o, int v,
                                                     double omega, int triplet, double *__restrict__ part, double *__restrict__ pmin)
{
    __shared__ double sA[TFD_T][TFD_P], sB[TFD_T][TFD_P];     // [b - b0][a - a0]: M[j][b][i][a] and M[i][b][j][a]
    __shared__ double s_sum[256], s_min[256];
    int i, j, a0, b0;
    tile_of_block(o, v, i, j, a0, b0);
    const long long dim = (long long)o * v;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TFD_T + tx;
    {
        const int a = a0 + tx, b = b0 + ty;                   // lanes along a
        if (a < v && b < v) {
            sA[ty][tx] = M[((long long)j * v + b) * dim + (long long)i * v + a];
            sB[ty][tx] = M[((long long)i * v + b) * dim + (long long)j * v + a];
        }
    }
    __syncthreads();
    const int a = a0 + ty, b = b0 + tx;                       // lanes along b
    double term = 0.0, dmin = INFINITY;
    if (a < v && b < v) {
        const double m_iajb = M[((long long)i * v + a) * dim + (long long)j * v + b];
        const double m_jaib = M[((long long)j * v + a) * dim + (long long)i * v + b];
        const double m_jbia = sA[tx][ty], m_ibja = sB[tx][ty];
        const double uS = m_iajb + m_jbia, uSx = m_jaib + m_ibja, uT = m_iajb - m_jbia;
        const double den = ((eps[n_frozen + i] + eps[n_frozen + j]) - (eps[n_occ + a] + eps[n_occ + b])) + omega;
        term = triplet ? 0.5 * ((uS * uS - uS * uSx) + uT * uT) / den : uS * (uS - 0.5 * uSx) / den;
        dmin = fabs(den);
    }
    s_sum[tid] = term; s_min[tid] = dmin;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            s_sum[tid] += s_sum[tid + s];
            if (s_min[tid + s] < s_min[tid]) s_min[tid] = s_min[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) { part[blockIdx.x] = s_sum[0]; pmin[blockIdx.x] = s_min[0]; }
}

inline void launch_operands(const double *g, const double *eps, int n_frozen, int n_occ, int o, int v, double *t, double *tt, double *L, hipStream_t st)
{
    hipLaunchKernelGGL(operands_kernel, dim3((unsigned)tile_blocks(o, v)), dim3(TFD_T, TFD_T), 0, st, g, eps, n_frozen, n_occ, o, v, t, tt, L);
}

inline void launch_direct(const double *M, const double *eps, int n_frozen, int n_occ, int o, int v, double omega, int triplet, double *part, double *pmin,
                          hipStream_t st)
{
    hipLaunchKernelGGL(direct_kernel, dim3((unsigned)tile_blocks(o, v)), dim3(TFD_T, TFD_T), 0, st, M, eps, n_frozen, n_occ, o, v, omega, triplet, part, pmin);
}

}  // namespace tfcisd
