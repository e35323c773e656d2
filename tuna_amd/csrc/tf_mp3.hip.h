// tf_mp3.hip.h -- restricted MP3 on the HBM-resident tensor (run_restricted_MP3, tuna_mp.py:1410-1470).
// Notation: occupied window i, j, k, l (o orbitals), virtual window a, b, c, d (v orbitals), D = e_i + e_j - e_a - e_b,
//     t_ijab = (ia|jb) / D,   t'_ijab = 2 [2 (ia|jb) - (ib|ja)] / D,   E_MP3 = sum t'_ijab X_ijab,
//     X = 1/2 sum_cd t_ijcd (ac|bd)  (pp)  +  1/2 sum_kl t_klab (ki|lj)  (hh)
//       + sum_kc t_ikac [2 (bj|kc) - (bc|kj)] - sum_kc t_kjac (bc|ki) - sum_kc t_kiac (bj|kc)   (ring).
// Every term but pp uses blocks of o^2 v^2 or fewer values, made by the AO->MO transformation (tf_mp2.hip.h) and contracted by
// rocBLAS GEMMs.  The particle-particle ladder never forms (ac|bd) (v^4: 170 GB at N = 400): with the AO pair matrices
// T_ij = C_v t_ij C_v^T it is 1/2 C_v^T Z_ij C_v, Z_ij[mu][nu] = sum_{lambda sigma} (mu lambda|nu sigma) T_ij[lambda][sigma] -- an
// exchange-type contraction of the tensor with o^2 general matrices.  On the packed layout mp3_ladder_kernel streams the stored
// rows once per batch of pairs (the pairs are the B columns of the FP64 matrix core); on the other layouts Z_ij comes from the
// general-density exchange build (the caller, tf_device.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "tf_jkpacked.hip.h"
#include "tf_mp2.hip.h"

namespace tfmp3 {

using tfmp2::tfm_v4d;

// Amplitudes and the MP2 partials in one pass over g[i][a][j][b] = (ia|jb) (the loop and the reduction of tfmp2::mp2_energy_kernel,
// so that the MP2 partials are bit for bit those of tf_mp2_rhf):
//     tov[i][a][j][b] = t_ijab                 (the ring GEMMs' left operand: t_ikac as [(ia)][(kc)])
//     too[i][j][a][b] = t_ijab                 (the pair matrices of the ladders)
//     tp [i][j][a][b] = t'_ijab
//     tsw[j][a][i][b] = t_ijab                 (t_kjac as [(ja)][(kc)])
__global__ void mp3_amp_kernel(const double *__restrict__ g, const double *__restrict__ eps, int n_frozen, int o, int v, int n_occ_total,
                               double *__restrict__ tov, double *__restrict__ too, double *__restrict__ tp, double *__restrict__ tsw,
                               double *__restrict__ partial /* [gridDim.x][2] */)
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
        const double t = gij / D;
        const long long ijab = (((long long)i * o + j) * v + a) * v + b;
        tov[e] = t;
        too[ijab] = t;
        tp[ijab] = 2.0 * (2.0 * gij - gx) / D;
        tsw[(((long long)j * v + a) * o + i) * v + b] = t;
    }
    s_os[threadIdx.x] = os; s_ss[threadIdx.x] = ss;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s_os[threadIdx.x] += s_os[threadIdx.x + s]; s_ss[threadIdx.x] += s_ss[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s_os[0]; partial[2 * blockIdx.x + 1] = s_ss[0]; }
}

// The GEMM operands of the hole-hole and ring terms, from (ki|lj) = g3[k][i][l][j], (ia|jb) = g1[i][a][j][b], (ab|ij) = g2[a][b][i][j]:
//     Moo[(ij)][(kl)] = (ki|lj),   M1[(kc)][(jb)] = 2 (kc|jb) - (kj|bc),   M2[(kc)][(ib)] = (ki|bc)
__global__ void mp3_operands_kernel(const double *__restrict__ g1, const double *__restrict__ g2, const double *__restrict__ g3, int o, int v,
                                    double *__restrict__ Moo, double *__restrict__ M1, double *__restrict__ M2)
{
    const long long ov = (long long)o * v, n2 = ov * ov, n4 = (long long)o * o * o * o, total = n2 > n4 ? n2 : n4;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        if (e < n2) {
            const long long kc = e / ov, jb = e - kc * ov;
            const int k = (int)(kc / v), c = (int)(kc - (long long)k * v);
            const int j = (int)(jb / v), b = (int)(jb - (long long)j * v);
            const double g2v = g2[(((long long)b * v + c) * o + k) * o + j];   // (kj|bc)
            M1[e] = 2.0 * g1[e] - g2v;
            M2[e] = g2v;                                              // (the (ib) column of M2 is this (jb))
        }
        if (e < n4) {
            long long r = e;
            const int l = (int)(r % o); r /= o;
            const int kk = (int)(r % o); r /= o;
            const int jj = (int)(r % o);
            const int ii = (int)(r / o);
            Moo[e] = g3[(((long long)kk * o + ii) * o + l) * o + jj];   // Moo[ii jj][kk l] = (kk ii|l jj)
        }
    }
}

// Tt[lambda][sigma][p] = T[p][lambda][sigma] for p < nb, zero for nb <= p < TFL_W: the pair index becomes the fastest (the B columns
// of the ladder kernel)
#define TFL_W 64                  // pairs of a batch: four MFMA column tiles
__global__ void mp3_pairs_last_kernel(const double *__restrict__ T, int N, int nb, double *__restrict__ Tt)
{
    const long long nn = (long long)N * N, total = nn * TFL_W;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long ls = e / TFL_W;
        const int p = (int)(e - ls * TFL_W);
        Tt[e] = p < nb ? T[(long long)p * nn + ls] : 0.0;
    }
}

// ---- the particle-particle ladder on the packed rows -------------------------------------------------------------------------------
// Zh[p][mu][nu] = sum_lambda sum_sigma R_(mu lambda)[nu][sigma] T_p[lambda][sigma]     (internal AO order, p < TFL_W pairs of a batch)
// R_(mu lambda) = the stored part of row (max, min) expanded to a symmetric matrix, the pair equal to the row's own halved (the
// convention of tfmp2::mo_q1_kernel); Zh is then the contraction with the stored triangle L, and Z_p = Zh_p + Zh_{p'}^T where p' is
// the transposed pair (T_ji = T_ij^T: the caller adds the two after the back-transformation).
//   * one workgroup per (bra AO mu, group of 16-row blocks nu of one parity class); wave w owns TFL_MB blocks of the group and keeps
//     their 16 x 64 tiles in registers while the workgroup walks lambda = 0 .. N - 1 (internal order) through the row map: one owner
//     per output element, a fixed order of summation, no atomics -- bitwise reproducible.  Every stored value is read twice, once per
//     bra index of its row.
//   * per lambda the workgroup builds the segment table of row (mu lambda) in LDS (as mo_q1_kernel does per row); a block then takes
//     the "row" image (its own 16 segments, all their columns) and the "column" image (the segments that reach its 16 columns) on
//     v_mfma_f64_16x16x4_f64 with A = the row's values (global memory straight into the lane layout) and B = Tt[lambda][sigma][p]
//     (128 contiguous bytes per 16-lane row; the 200 KB of one lambda are shared by all blocks of the workgroup through the caches).
#define TFL_THREADS 512
#define TFL_MB 2                  // blocks per wave: 8 accumulator tiles (32 doubles) per lane
struct LadderArgs {
    const double *eri;
    const long long *rowoff;
    const int *rowsec;
    const int2 *row_ij;
    const int *rowmap;            // keyed by internal pairs (hi (hi + 1) / 2 + lo): local row, -1 = absent
    const double *Tt;             // [N lambda][N sigma][TFL_W]
    double *Zh;                   // [TFL_W][N mu][N nu]
    int nb;                       // pairs of this batch (<= TFL_W): the columns that are stored
    int nblk;                     // 16-row blocks of all classes
};

__global__ __launch_bounds__(TFL_THREADS) void mp3_ladder_kernel(LadderArgs A, BLayout L)
{
    extern __shared__ int2 sSeg[];                                   // [N]: per internal AO k, offset of its segment in the row; values it holds
    const int N = L.N;
    const int mu = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = lane & 15, kk = lane >> 4;
    constexpr int NT = TFL_W / 16;
    constexpr int NW = TFL_THREADS / 64;
    int bfirst[5];
    bfirst[0] = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) bfirst[x + 1] = bfirst[x] + (L.itab[BL_CSIZE + x] + 15) / 16;
    tfm_v4d acc[TFL_MB][NT];
#pragma unroll
    for (int q = 0; q < TFL_MB; ++q)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[q][t] = tfm_v4d{0.0, 0.0, 0.0, 0.0};
    for (int lamI = 0; lamI < N; ++lamI) {
        const int hi = max(mu, lamI), lo = min(mu, lamI);
        const int r = A.rowmap[(size_t)hi * (hi + 1) / 2 + lo];
        if (r < 0) continue;                                         // (uniform over the workgroup)
        const int2 ij = A.row_ij[r];
        const int wi = L.ao[ij.x], wj = L.ao[ij.y];
        const int c = ao_cls(wi) ^ ao_cls(wj), iI = ao_sigma(L, wi), lamj = ao_loc(wj);
        const double *__restrict__ T = A.eri + A.rowoff[r];
        const int *rs = A.rowsec + 6 * (size_t)r;
        __syncthreads();                                             // the previous row's table is no longer read
        // segment table: AOs beyond i (original order) hold nothing, the segment of k == i ends at l == j
        for (int kI = threadIdx.x; kI < N; kI += TFL_THREADS) {
            const int a = L.clsI[kI];
            const KInfo ki = L.kinfo[(size_t)c * N + kI];
            const int pc = (ki.cnt + TF_SEG_PAD - 1) & ~(TF_SEG_PAD - 1);
            const bool have = kI - bl_cstart(L, a) < L.cntA[(size_t)a * N + iI];
            sSeg[kI] = make_int2(rs[5] * (rs[a] + ki.offA) + rs[4] * pc, have ? (kI == iI ? lamj + 1 : ki.cnt) : 0);
        }
        __syncthreads();
        const double *__restrict__ Tb = A.Tt + (size_t)lamI * N * TFL_W;
        const bool diag_cls = c == 0;                                // l and k of one class: l == k <=> lam == kl
#pragma unroll
        for (int q = 0; q < TFL_MB; ++q) {
            const int blk = blockIdx.y * (NW * TFL_MB) + w + NW * q;
            if (blk >= A.nblk) continue;
            const int x = blk >= bfirst[3] ? 3 : (blk >= bfirst[2] ? 2 : (blk >= bfirst[1] ? 1 : 0));
            const int s0 = 16 * (blk - bfirst[x]);
            const int x0 = bl_cstart(L, x);
            const int a = x ^ c, a0 = bl_cstart(L, a), na = L.itab[BL_CSIZE + a];
            // ---- row image: the block's own segments k = s0 .. s0 + 15 of class x, all their columns l of class a, l != k
            const int klimR = L.cntA[(size_t)x * N + iI];
            const bool have_row = s0 < klimR;
            const int klR = s0 + m;
            const bool vkR = have_row && klR < klimR;
            const int kIR = x0 + (vkR ? klR : 0);
            const int2 sgR = sSeg[kIR];
            const int pcR = vkR ? ((sgR.y + TF_SEG_PAD - 1) & ~(TF_SEG_PAD - 1)) : 0;   // (slots between cnt and the pad hold zeros)
            const double *__restrict__ segR = T + sgR.x;
            int cmax = 0;                                            // the longest segment of the block: its last one, or -- the segment
            if (have_row) {                                          // of k == i being cut at l == j -- the one before
                const int last = min(s0 + 15, klimR - 1);
                cmax = sSeg[x0 + last].y;
                if (last > s0) cmax = max(cmax, sSeg[x0 + last - 1].y);
            }
            for (int l0 = 0; l0 < cmax; l0 += 32) {
                const int lb = l0 + 8 * kk;                          // this lane's eight columns
                double v[8];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool in = lb + 2 * u < pcR;
                    const double2 t2 = in ? *reinterpret_cast<const double2 *>(segR + lb + 2 * u) : make_double2(0.0, 0.0);
                    v[2 * u] = t2.x; v[2 * u + 1] = t2.y;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int lam = lb + u;
                    if (lam >= sgR.y || (diag_cls && lam == klR)) v[u] = 0.0;
                    if (kIR == iI && lam == lamj) v[u] *= 0.5;
                    const bool vl = lam < na;
                    const double *bp = Tb + (size_t)(a0 + (vl ? lam : 0)) * TFL_W + m;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const double bv = vl ? bp[16 * t] : 0.0;
                        acc[q][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], bv, acc[q][t], 0, 0, 0);
                    }
                }
            }
            // ---- column image: the segments k of class a that reach the columns s0 .. s0 + 15 of class x; a lane takes eight
            //      consecutive k per pass.  First member: the first segment longer than s0 (cnt is non-decreasing, except that the
            //      segment of k == i -- the last member when i is of class a -- is cut at l == j: it stays out of the search).
            const int klim = L.cntA[(size_t)a * N + iI];
            int lo_col = 0, hi_col = (klim > 0 && a0 + klim - 1 == iI) ? klim - 1 : klim;
            while (lo_col < hi_col) { const int mid = (lo_col + hi_col) >> 1; if (sSeg[a0 + mid].y > s0) hi_col = mid; else lo_col = mid + 1; }
            const int lam = s0 + m;
            for (int kl0 = lo_col & ~7; kl0 < klim; kl0 += 32) {
                double v[8];
                int kIs[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int kl = kl0 + 8 * kk + u;
                    const bool vk = kl < klim;
                    const int kI = a0 + (vk ? kl : 0);
                    const int2 sg = sSeg[kI];
                    const bool ok = vk && lam < sg.y;
                    v[u] = ok ? __builtin_nontemporal_load(T + sg.x + lam) : 0.0;
                    kIs[u] = vk ? kI : -1;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (kIs[u] == iI && lam == lamj) v[u] *= 0.5;
                    const double *bp = Tb + (size_t)(kIs[u] >= 0 ? kIs[u] : 0) * TFL_W + m;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const double bv = kIs[u] >= 0 ? bp[16 * t] : 0.0;
                        acc[q][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], bv, acc[q][t], 0, 0, 0);
                    }
                }
            }
        }
    }
    // ---- the tiles: rows nu = x0 + s0 + 4 v + (lane >> 4), columns p = 16 t + (lane & 15)
#pragma unroll
    for (int q = 0; q < TFL_MB; ++q) {
        const int blk = blockIdx.y * (NW * TFL_MB) + w + NW * q;
        if (blk >= A.nblk) continue;
        const int x = blk >= bfirst[3] ? 3 : (blk >= bfirst[2] ? 2 : (blk >= bfirst[1] ? 1 : 0));
        const int s0 = 16 * (blk - bfirst[x]);
        const int x0 = bl_cstart(L, x), nx = L.itab[BL_CSIZE + x];
#pragma unroll
        for (int vv = 0; vv < 4; ++vv) {
            const int row = s0 + 4 * vv + kk;
            if (row >= nx) continue;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int p = 16 * t + m;
                if (p < A.nb) A.Zh[((size_t)p * N + mu) * N + x0 + row] = acc[q][t][vv];
            }
        }
    }
}

// E_MP3 per term: partial[block][3] = sum t'_ijab X_ijab over the block's share of (ijab), in the order of a fixed grid (the caller sums
// the blocks in block order: bitwise reproducible).
//     pp:   X = Y[ij][a][b] (+ Y[ji][b][a] when Y holds the back-transformed Zh of the stored triangle: Z_ij = Zh_ij + Zh_ji^T)
//     hh:   X = Xhh[ij][ab]
//     ring: X = S13[(ia)][(jb)] - S2[(ja)][(ib)]
__global__ void mp3_energy_kernel(const double *__restrict__ tp, const double *__restrict__ Y, int add_transposed, const double *__restrict__ Xhh,
                                  const double *__restrict__ S13, const double *__restrict__ S2, int o, int v, double *__restrict__ partial)
{
    __shared__ double s_e[3][256];
    const long long total = (long long)o * o * v * v;
    double e_pp = 0.0, e_hh = 0.0, e_ring = 0.0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int a = (int)(r % v); r /= v;
        const int j = (int)(r % o);
        const int i = (int)(r / o);
        const double t = tp[e];
        double pp = Y[e];
        if (add_transposed) pp += Y[(((long long)j * o + i) * v + b) * v + a];
        e_pp += t * pp;
        e_hh += t * Xhh[e];
        e_ring += t * (S13[(((long long)i * v + a) * o + j) * v + b] - S2[(((long long)j * v + a) * o + i) * v + b]);
    }
    s_e[0][threadIdx.x] = e_pp; s_e[1][threadIdx.x] = e_hh; s_e[2][threadIdx.x] = e_ring;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int q = 0; q < 3; ++q) s_e[q][threadIdx.x] += s_e[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int q = 0; q < 3; ++q) partial[3 * blockIdx.x + q] = s_e[q][0];
}

// Row-major GEMMs on rocBLAS (column-major): C[M][N] = alpha op(A) op(B) + beta C  <=>  C^T = op(B)^T op(A)^T
inline rocblas_status gemm_rm(rocblas_handle h, bool ta, bool tb, int M, int Nc, int K, double alpha, const double *A, int lda, const double *B,
                              int ldb, double beta, double *C, int ldc)
{
    return rocblas_dgemm(h, tb ? rocblas_operation_transpose : rocblas_operation_none, ta ? rocblas_operation_transpose : rocblas_operation_none,
                         Nc, M, K, &alpha, B, ldb, A, lda, &beta, C, ldc);
}
inline rocblas_status gemm_rm_batched(rocblas_handle h, bool ta, bool tb, int M, int Nc, int K, double alpha, const double *A, int lda,
                                      long long sa, const double *B, int ldb, long long sb, double beta, double *C, int ldc, long long sc, int batch)
{
    return rocblas_dgemm_strided_batched(h, tb ? rocblas_operation_transpose : rocblas_operation_none, ta ? rocblas_operation_transpose : rocblas_operation_none,
                                         Nc, M, K, &alpha, B, ldb, (rocblas_stride)sb, A, lda, (rocblas_stride)sa, &beta, C, ldc, (rocblas_stride)sc, batch);
}

// 16-row blocks of the four classes (the column count of the ladder kernel's grid needs it on the host)
inline int ladder_blocks(const int csize[4]) { int n = 0; for (int x = 0; x < 4; ++x) n += (csize[x] + 15) / 16; return n; }

inline void launch_ladder(const LadderArgs &A, const BLayout &BL, int N, hipStream_t st)
{
    const int groups = (A.nblk + (TFL_THREADS / 64) * TFL_MB - 1) / ((TFL_THREADS / 64) * TFL_MB);
    hipLaunchKernelGGL(mp3_ladder_kernel, dim3((unsigned)N, (unsigned)groups), dim3(TFL_THREADS), (size_t)N * sizeof(int2), st, A, BL);
}

}  // namespace tfmp3
