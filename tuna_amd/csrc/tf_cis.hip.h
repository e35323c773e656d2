// tf_cis.hip.h -- closed-shell CIS and TDHF (RPA) excited states on the HBM-resident tensor (calculate_A_matrix / calculate_B_matrix,
// tuna_ci.py:719-841; calculate_restricted_single_reference_excited_states, :1284-1366; calculate_restricted_transition_dipoles,
// :1466-1518).  Notation of tf_mp3.hip.h: occupied i, j (o orbitals), virtual a, b (v orbitals), dim = o v, compound index
// (ia) = i v + a, Delta = diag(e_a - e_i).  With G = (ia|jb), H = (ij|ab), X = (ib|ja), all [(ia)][(jb)]:
//     CIS:   A singlet = Delta + 2 G - H                A triplet = Delta - H
//     TDHF:  A + B singlet = Delta + 4 G - H - X        A + B triplet = Delta - H - X        A - B (both) = Delta - H + X
// each symmetrised as 1/2 (M + M^T) (tuna_util.py: symmetrise).  From the blocks of tf_mp3_rhf, (ia|jb) = g1[i][a][j][b] and
// (ab|ij) = g2[a][b][i][j]: G is g1 itself, X is g1 with a and b exchanged, and H is g2 with its index pairs in the opposite order.
//   * transpose_kernel turns g2 [(ab)][(ij)] into Ht [(ij)][(ab)] through a padded LDS tile, so that H runs along b as the output does;
//   * assemble_kernel writes every matrix of the call in one pass, a 32 x 32 tile of [(ia)][(jb)] per workgroup.  M[p][q] needs
//     G[p][q], X[q][p], Ht at (p, q) -- contiguous along q, read straight into registers -- and for the transposed image G[q][p],
//     X[p][q], Ht at (q, p) -- contiguous along p: read with p as the lane index into padded LDS tiles and picked up transposed.  Every
//     global read and write is a run of up to 32 consecutive doubles; no atomics; out[p][q] and out[q][p] are the same two terms added in
//     either order, so every matrix is symmetric to the last bit.
// TD-DFT / TDA (tf_tddft_rhf) is the same pass with H and X scaled by the share of exact exchange and the exchange-correlation kernel
// matrix of tf_xckernel.hip.h added per matrix: A gains K, A + B gains 2 K, A - B nothing (AssembleArgs::hfx, K, kfac).
// TDHF is solved through A - B = L L^T: (L^T (A + B) L) Z = w^2 Z, X + Y = L Z / sqrt(w), X - Y = sqrt(w) L^-T Z (the caller,
// tf_device.hip: rocSOLVER dpotrf and dsyevd, rocBLAS dtrmm and dtrsm), which gives X.X - Y.Y = (X + Y).(X - Y) = 1.  Every reduction
// is per block, the blocks summed in block order: bitwise repeatable.
#pragma once
#include <hip/hip_runtime.h>

namespace tfcis {

#define TFX_T 32                  // tile edge
#define TFX_P (TFX_T + 1)         // padded row of an LDS tile: a column walk touches 32 different banks

// out[c][r] = in[r][c] for in [rows][cols]: block (32, 8), grid (cols / 32, rows / 32) rounded up
__global__ void transpose_kernel(const double *__restrict__ in, long long rows, long long cols, double *__restrict__ out)
{
    __shared__ double s[TFX_T][TFX_P];
    const long long r0 = (long long)blockIdx.y * TFX_T, c0 = (long long)blockIdx.x * TFX_T;
    for (int y = threadIdx.y; y < TFX_T; y += 8) {
        const long long r = r0 + y, c = c0 + threadIdx.x;
        if (r < rows && c < cols) s[y][threadIdx.x] = in[r * cols + c];
    }
    __syncthreads();
    for (int y = threadIdx.y; y < TFX_T; y += 8) {
        const long long c = c0 + y, r = r0 + threadIdx.x;
        if (r < rows && c < cols) out[c * rows + r] = s[threadIdx.x][y];
    }
}

// One element before the symmetrisation, in one fixed order of its terms.  kind: 0 = A singlet, 1 = A triplet, 2 = A + B singlet,
// 3 = A + B triplet, 4 = A - B
__device__ __forceinline__ double cis_element(int kind, double delta, double G, double H, double X)
{
#pragma clang fp contract(off)    // both images of an element round alike wherever the call is inlined
    switch (kind) {
    case 0: return (delta + 2.0 * G) - H;
    case 1: return delta - H;
    case 2: return ((delta + 4.0 * G) - H) - X;
    case 3: return (delta - H) - X;
    default: return (delta - H) + X;
    }
}

struct AssembleArgs {
    const double *g1;             // [i][a][j][b] = (ia|jb)
    const double *Ht;             // [i][j][a][b] = (ij|ab)
    const double *eps;            // [N] orbital energies (device)
    int n_frozen, n_occ, o, v;
    int n_out;                    // matrices of this call (<= 3)
    int kind[3];
    double *out[3];               // [dim][dim] each
    // TD-DFT (tf_tddft_rhf): H and X enter scaled by hfx (Ht may be null when hfx = 0: the block is then neither built nor read), and
    // matrix m gains kfac[m] K[m] after the symmetrisation -- K [dim][dim] is symmetric to the last bit (tf_xckernel.hip.h).  The
    // defaults are Hartree-Fock: hfx = 1 multiplies exactly, a null K adds nothing.
    double hfx = 1.0;
    const double *K[3] = {nullptr, nullptr, nullptr};
    double kfac[3] = {0.0, 0.0, 0.0};
};

// block (32, 8), grid (dim / 32, dim / 32) rounded up: tile rows p0 .., columns q0 ..
__global__ __launch_bounds__(256) void assemble_kernel(AssembleArgs A)
{
    __shared__ double sG[TFX_T][TFX_P], sX[TFX_T][TFX_P], sH[TFX_T][TFX_P];     // [q - q0][p - p0]: G[q][p], X[p][q], H at (q, p)
    const int o = A.o, v = A.v;
    const long long dim = (long long)o * v;
    const long long p0 = (long long)blockIdx.y * TFX_T, q0 = (long long)blockIdx.x * TFX_T;
    const int tx = threadIdx.x;
    // ---- the transposed image: lane index along p
    {
        const long long p = p0 + tx;
        const int i = (int)(p / v), a = (int)(p - (long long)i * v);
        for (int y = threadIdx.y; y < TFX_T; y += 8) {
            const long long q = q0 + y;
            if (p < dim && q < dim) {
                const int j = (int)(q / v), b = (int)(q - (long long)j * v);
                sG[y][tx] = A.g1[q * dim + p];
                sX[y][tx] = A.g1[((long long)i * v + b) * dim + (long long)j * v + a];                  // (ib|ja)
                sH[y][tx] = A.Ht ? A.Ht[(((long long)j * o + i) * v + b) * v + a] : 0.0;                // (ji|ba)
            }
        }
    }
    __syncthreads();
    // ---- the direct image and the output: lane index along q
    const long long q = q0 + tx;
    if (q >= dim) return;
    const int j = (int)(q / v), b = (int)(q - (long long)j * v);
    for (int y = threadIdx.y; y < TFX_T; y += 8) {
        const long long p = p0 + y;
        if (p >= dim) break;
        const int i = (int)(p / v), a = (int)(p - (long long)i * v);
        const double G = A.g1[p * dim + q];
        const double X = sX[tx][y];                                                                      // (ib|ja) = X[p][q]
        const double H = A.Ht ? A.Ht[(((long long)i * o + j) * v + a) * v + b] : 0.0;
        const double Gt = sG[tx][y];
        const double Xt = A.g1[((long long)j * v + a) * dim + (long long)i * v + b];                     // (ja|ib) = X[q][p]
        const double Hq = sH[tx][y];
        const double delta = p == q ? A.eps[A.n_occ + a] - A.eps[A.n_frozen + i] : 0.0;
        const double hH = A.hfx * H, hX = A.hfx * X, hHq = A.hfx * Hq, hXt = A.hfx * Xt;
        for (int m = 0; m < A.n_out; ++m) {
            double r = 0.5 * (cis_element(A.kind[m], delta, G, hH, hX) + cis_element(A.kind[m], delta, Gt, hHq, hXt));
            if (A.K[m]) r += A.kfac[m] * A.K[m][p * dim + q];
            A.out[m][p * dim + q] = r;
        }
    }
}

// The roots of the reduced TDHF problem: w[n] = sqrt(w2[n]) (0 where w2[n] <= 0 or not finite), stat[0] = the number of such roots,
// stat[1] = the smallest w2.  One block of 256 threads, a strided share per thread, the shares combined in a fixed tree.
__global__ void tdhf_roots_kernel(const double *__restrict__ w2, int dim, double *__restrict__ w, double *__restrict__ stat)
{
    __shared__ double s_min[256];
    __shared__ int s_bad[256];
    double mn = INFINITY;
    int bad = 0;
    for (int n = threadIdx.x; n < dim; n += 256) {
        const double x = w2[n];
        const bool ok = x > 0.0 && isfinite(x);
        if (!ok) ++bad;
        if (!(x >= mn)) mn = x;                                       // (a NaN is kept: it is the offending value)
        w[n] = ok ? sqrt(x) : 0.0;
    }
    s_min[threadIdx.x] = mn; s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            if (!(s_min[threadIdx.x + s] >= s_min[threadIdx.x])) s_min[threadIdx.x] = s_min[threadIdx.x + s];
            s_bad[threadIdx.x] += s_bad[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { stat[0] = (double)s_bad[0]; stat[1] = s_min[0]; }
}

// TDHF back-substitution, state n = column n (contiguous, dim values): P[n] = L Z_n becomes X + Y = P[n] / sqrt(w_n) for every state;
// for the kept states n < n_keep, with Q[n] = L^-T Z_n: X - Y = sqrt(w_n) Q[n], X = 1/2 [(X + Y) + (X - Y)], Y = 1/2 [(X + Y) - (X - Y)]
__global__ void tdhf_backsub_kernel(double *__restrict__ P, const double *__restrict__ Q, const double *__restrict__ w, int dim, int n_keep,
                                    double *__restrict__ Xk, double *__restrict__ Yk)
{
    const long long total = (long long)dim * dim;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(e / dim);
        const double r = sqrt(w[n]);
        const double xpy = P[e] / r;
        P[e] = xpy;
        if (n < n_keep) {
            const double xmy = r * Q[e];
            Xk[e] = 0.5 * (xpy + xmy);
            Yk[e] = 0.5 * (xpy - xmy);
        }
    }
}

// f_n = (2/3) w_n |mu_n|^2 from mu [dim][3]
__global__ void oscillator_kernel(const double *__restrict__ mu, const double *__restrict__ w, int dim, double *__restrict__ f)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= dim) return;
    const double x = mu[3 * n], y = mu[3 * n + 1], z = mu[3 * n + 2];
    f[n] = (2.0 / 3.0) * w[n] * ((x * x + y * y) + z * z);
}

inline void launch_transpose(const double *in, long long rows, long long cols, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + TFX_T - 1) / TFX_T), (unsigned)((rows + TFX_T - 1) / TFX_T)), dim3(TFX_T, 8), 0, st, in,
                       rows, cols, out);
}

inline void launch_assemble(const AssembleArgs &A, hipStream_t st)
{
    const long long dim = (long long)A.o * A.v;
    const unsigned nt = (unsigned)((dim + TFX_T - 1) / TFX_T);
    hipLaunchKernelGGL(assemble_kernel, dim3(nt, nt), dim3(TFX_T, 8), 0, st, A);
}

}  // namespace tfcis
