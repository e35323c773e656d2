// tf_xckernel.hip.h -- the matrix elements of the exchange-correlation kernel for closed-shell TD-DFT / TDA
// (calculate_restricted_exchange_correlation_kernel_matrices, tuna_dft.py:1097-1147):
//     K_S[(ia)][(jb)] = sum_g u_S(g) psi_i(g) psi_a(g) psi_j(g) psi_b(g),     K_T likewise with u_T,
// u = w (DFX f_X + DFC f_C) per grid point (tfdft::xc_fpoint_kernel), compound index (ia) = i v + a as in tf_cis.hip.h.  A symmetric
// rank-G update whose operand, the transition density T[(ia)][g] = psi_i(g) psi_a(g) (dim x G: 5.5 GB at N = 400, o = 18 and 10^5
// points), is never written to memory: it is formed in LDS, chunk by chunk, from psi [G][o + v].
//   * xck_kernel: one workgroup per (tile, slab).  A tile is 64 x 64 elements of K with row block <= column block; a slab is a
//     contiguous run of grid points (tf_xckernel_plan.h).  Per chunk of XCK_CHUNK points the workgroup stages the left operand
//     T[p0 .. p0 + 63][g], the right operand T[q0 .. q0 + 63][g] and u_S, u_T in LDS ([g][row], XCK_ROW doubles per point: the lanes of a
//     wave write and read 16 consecutive doubles per k-row, and 80 = 16 (mod 32) keeps the k-rows of one read on different banks).
//     Wave w owns the rows 16 w .. 16 w + 15 of the tile: per four grid points one read of the left operand (A[m][k], lane = 16 k + m)
//     feeds eight v_mfma_f64_16x16x4_f64 -- four column blocks times the two accumulator sets, whose right operands are the same staged
//     value scaled by u_S and by u_T.  Rows and columns past dim and points past the slab are staged as zeros.
//   * the tile's elements with p <= q go to the slab's partial [slab][S | T][p][q]; xck_sum_kernel adds the slabs in slab order and writes
//     K[p][q] and K[q][p] from the one sum: symmetric to the last bit.  No atomics; the order of every sum is fixed by the plan, which
//     depends on (dim, G) alone.
#pragma once
#include <hip/hip_runtime.h>

#include "tf_mp2.hip.h"
#include "tf_xckernel_plan.h"

namespace tfxck {

using tfmp2::tfm_v4d;

struct Args {
    const double *psi;            // [G][n]: columns 0 .. o - 1 the occupied window, o .. o + v - 1 the virtual window
    const double *uS, *uT;        // [G]
    double *part;                 // [n_slabs][2][dim][dim]
    long long G, slab_len;
    int n, o, v, dim, n_b;
};

// blockIdx.x = tile (row block bi <= column block bj, listed row by row), blockIdx.y = slab
__global__ __launch_bounds__(XCK_THREADS) void xck_kernel(Args A)
{
    __shared__ double sL[XCK_CHUNK * XCK_ROW], sR[XCK_CHUNK * XCK_ROW], sUS[XCK_CHUNK], sUT[XCK_CHUNK];
    // tile -> (bi, bj): row bi of the upper triangle starts at bi n_b - bi (bi - 1) / 2
    int bi = 0, t = blockIdx.x;
    while (t >= A.n_b - bi) { t -= A.n_b - bi; ++bi; }
    const int bj = bi + t;
    const int p0 = bi * XCK_TILE, q0 = bj * XCK_TILE;
    const long long g_first = (long long)blockIdx.y * A.slab_len;
    const long long g_last = g_first + A.slab_len < A.G ? g_first + A.slab_len : A.G;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = lane & 15, kk = lane >> 4;
    // staging: thread = (row r of the tile, quarter gq of the chunk's points); the orbitals of its row and of its column
    const int r = threadIdx.x & 63, gq = threadIdx.x >> 6;
    const int p = p0 + r, q = q0 + r;
    const bool vp = p < A.dim, vq = q < A.dim;
    const int pi = vp ? p / A.v : 0, pa = A.o + (vp ? p - pi * A.v : 0);
    const int qi = vq ? q / A.v : 0, qa = A.o + (vq ? q - qi * A.v : 0);
    constexpr int NT = XCK_TILE / 16;
    tfm_v4d accS[NT], accT[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) { accS[c] = tfm_v4d{0.0, 0.0, 0.0, 0.0}; accT[c] = tfm_v4d{0.0, 0.0, 0.0, 0.0}; }
    for (long long g0 = g_first; g0 < g_last; g0 += XCK_CHUNK) {
        __syncthreads();                                             // the previous chunk is no longer read
#pragma unroll
        for (int gl = gq; gl < XCK_CHUNK; gl += XCK_THREADS / 64) {
            const long long g = g0 + gl;
            const bool in = g < g_last;
            const double *row = A.psi + (in ? g : g_first) * A.n;
            sL[gl * XCK_ROW + r] = in && vp ? row[pi] * row[pa] : 0.0;
            sR[gl * XCK_ROW + r] = in && vq ? row[qi] * row[qa] : 0.0;
        }
        if (threadIdx.x < XCK_CHUNK) {
            const long long g = g0 + threadIdx.x;
            sUS[threadIdx.x] = g < g_last ? A.uS[g] : 0.0;
            sUT[threadIdx.x] = g < g_last ? A.uT[g] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < XCK_CHUNK; k0 += 4) {
            const int gl = k0 + kk;
            const double a = sL[gl * XCK_ROW + 16 * w + m];
            const double us = sUS[gl], ut = sUT[gl];
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const double b = sR[gl * XCK_ROW + 16 * c + m];
                accS[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b * us, accS[c], 0, 0, 0);
                accT[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b * ut, accT[c], 0, 0, 0);
            }
        }
    }
    // ---- the tile: rows p0 + 16 w + 4 vv + (lane >> 4), columns q0 + 16 c + (lane & 15); the upper triangle only
    const size_t dd = (size_t)A.dim * A.dim;
    double *outS = A.part + (size_t)blockIdx.y * 2 * dd, *outT = outS + dd;
#pragma unroll
    for (int vv = 0; vv < 4; ++vv) {
        const int row = p0 + 16 * w + 4 * vv + kk;
        if (row >= A.dim) continue;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int col = q0 + 16 * c + m;
            if (col >= A.dim || col < row) continue;
            outS[(size_t)row * A.dim + col] = accS[c][vv];
            outT[(size_t)row * A.dim + col] = accT[c][vv];
        }
    }
}

// K[p][q] = K[q][p] = sum over the slabs, in slab order, of part[slab][.][p][q] for p <= q; thread = (p, q) of the full square, the
// lower triangle idle (the mirrored store of its partner covers it)
__global__ void xck_sum_kernel(const double *__restrict__ part, int n_slabs, int dim, double *__restrict__ KS, double *__restrict__ KT)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long dd = (long long)dim * dim;
    if (e >= dd) return;
    const int p = (int)(e / dim), q = (int)(e - (long long)p * dim);
    if (q < p) return;
    double s = 0.0, t = 0.0;
    for (int k = 0; k < n_slabs; ++k) { s += part[(size_t)k * 2 * dd + e]; t += part[(size_t)k * 2 * dd + dd + e]; }
    KS[e] = s; KT[e] = t;
    KS[(size_t)q * dim + p] = s; KT[(size_t)q * dim + p] = t;
}

// ---- the spin-blocked build: K of an unrestricted reference (calculate_unrestricted_exchange_correlation_kernel_matrices,
// tuna_dft.py:1194-1281), compound index = the alpha block then the beta block (tf_ucis.hip.h):
//     K[p][q] = sum_g u_st(g) psi_i^s(g) psi_a^s(g) psi_j^t(g) psi_b^t(g),     s the spin of p, t the spin of q.
// Blocks of XCK_TILE are cut per spin (XckSpinPlan), and a tile is one row block times NC adjacent column blocks of ONE spin, so it has one
// pair of spins: its left operand is staged from psi of s, its right operand from psi of t, its weight is u_aa, u_ab or u_bb.  The tiles
// come from the plan's list (xck_spin_tiles: those with an element row <= column; the beta-alpha rectangle is the transpose of alpha-beta
// and is never computed).  Staging, LDS layout and the wave's strip are xck_kernel's; there is one accumulator set, and with NC = 2
// (64 x 128: the registers the second set freed) one read of the left operand feeds eight matrix-core instructions and the left operand
// is staged once per 128 columns.  Every element is the same sequence of operations on the same values for either NC: the same bits.

struct SpinArgs {
    const double *psi[2];         // per spin [G][n_s]: columns 0 .. o_s - 1 the occupied window, then the virtual window
    const double *u[3];           // [G] each: u_aa, u_ab, u_bb
    const int *tiles;             // [n_tiles][3] = row block, first column block, column blocks (XckSpinTile)
    double *part;                 // [n_slabs][dim][dim]
    long long G, slab_len;
    int n[2], o[2], v[2], d[2], n_b[2];
    int dim;
};

// blockIdx.x = tile of the plan's list, blockIdx.y = slab
template <int NC>
__global__ __launch_bounds__(XCK_THREADS) void xck_spin_kernel(SpinArgs A)
{
    constexpr int RROW = NC * XCK_TILE + 16;                         // doubles between the grid points of the right operand: 16 (mod 32)
    __shared__ double sL[XCK_CHUNK * XCK_ROW], sR[XCK_CHUNK * RROW], sU[XCK_CHUNK];
    const int bi = A.tiles[3 * blockIdx.x], bj = A.tiles[3 * blockIdx.x + 1], nc = A.tiles[3 * blockIdx.x + 2];
    const int si = bi >= A.n_b[0], sj = bj >= A.n_b[0];           // si <= sj; all nc column blocks have spin sj
    const int p0 = (bi - (si ? A.n_b[0] : 0)) * XCK_TILE, q0 = (bj - (sj ? A.n_b[0] : 0)) * XCK_TILE;   // within the spin's part
    const double *psiL = A.psi[si], *psiR = A.psi[sj], *u = A.u[si + sj];
    const int nL = A.n[si], nR = A.n[sj];
    const long long g_first = (long long)blockIdx.y * A.slab_len;
    const long long g_last = g_first + A.slab_len < A.G ? g_first + A.slab_len : A.G;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = lane & 15, kk = lane >> 4;
    const int r = threadIdx.x & 63, gq = threadIdx.x >> 6;
    const int p = p0 + r;
    const bool vp = p < A.d[si];
    const int pi = vp ? p / A.v[si] : 0, pa = A.o[si] + (vp ? p - pi * A.v[si] : 0);
    bool vq[NC];
    int qi[NC], qa[NC];
#pragma unroll
    for (int b = 0; b < NC; ++b) {                                   // (columns past the spin's part, and the second block of a narrow tile: zeros)
        const int q = q0 + b * XCK_TILE + r;
        vq[b] = b < nc && q < A.d[sj];
        qi[b] = vq[b] ? q / A.v[sj] : 0;
        qa[b] = A.o[sj] + (vq[b] ? q - qi[b] * A.v[sj] : 0);
    }
    constexpr int NT = NC * XCK_TILE / 16;
    tfm_v4d acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = tfm_v4d{0.0, 0.0, 0.0, 0.0};
    for (long long g0 = g_first; g0 < g_last; g0 += XCK_CHUNK) {
        __syncthreads();                                             // the previous chunk is no longer read
#pragma unroll
        for (int gl = gq; gl < XCK_CHUNK; gl += XCK_THREADS / 64) {
            const long long g = g0 + gl;
            const bool in = g < g_last;
            const long long gr = in ? g : g_first;
            const double *rowL = psiL + gr * nL, *rowR = psiR + gr * nR;
            sL[gl * XCK_ROW + r] = in && vp ? rowL[pi] * rowL[pa] : 0.0;
#pragma unroll
            for (int b = 0; b < NC; ++b) sR[gl * RROW + b * XCK_TILE + r] = in && vq[b] ? rowR[qi[b]] * rowR[qa[b]] : 0.0;
        }
        if (threadIdx.x < XCK_CHUNK) {
            const long long g = g0 + threadIdx.x;
            sU[threadIdx.x] = g < g_last ? u[g] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < XCK_CHUNK; k0 += 4) {
            const int gl = k0 + kk;
            const double a = sL[gl * XCK_ROW + 16 * w + m];
            const double ug = sU[gl];
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const double b = sR[gl * RROW + 16 * c + m];
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b * ug, acc[c], 0, 0, 0);
            }
        }
    }
    // ---- the tile in the compound index: rows offL + p0 + ..., columns offR + q0 + ...; elements with row <= column only
    const int offL = si ? A.d[0] : 0, offR = sj ? A.d[0] : 0;
    double *out = A.part + (size_t)blockIdx.y * (size_t)A.dim * A.dim;
#pragma unroll
    for (int vv = 0; vv < 4; ++vv) {
        const int rl = p0 + 16 * w + 4 * vv + kk;
        if (rl >= A.d[si]) continue;
        const int row = offL + rl;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int cl = q0 + 16 * c + m;
            if (16 * c >= nc * XCK_TILE || cl >= A.d[sj]) continue;
            const int col = offR + cl;
            if (col < row) continue;
            out[(size_t)row * A.dim + col] = acc[c][vv];
        }
    }
}

// K[p][q] = K[q][p] = sum over the slabs, in slab order, of part[slab][p][q] for p <= q
__global__ void xck_spin_sum_kernel(const double *__restrict__ part, int n_slabs, int dim, double *__restrict__ K)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long dd = (long long)dim * dim;
    if (e >= dd) return;
    const int p = (int)(e / dim), q = (int)(e - (long long)p * dim);
    if (q < p) return;
    double s = 0.0;
    for (int k = 0; k < n_slabs; ++k) s += part[(size_t)k * dd + e];
    K[e] = s;
    K[(size_t)q * dim + p] = s;
}

}  // namespace tfxck
