// tf_scf.hip.h -- the restricted SCF cycle, resident on the GPU: J/K from the stored tensor (tf_kernels),
// rocBLAS for the O(N^3) products, rocSOLVER dsyevd for the symmetric eigenproblem; only scalars and the
// tiny DIIS system touch the host.
// Reference: run_restricted_SCF_cycle scf:1072-1154, run_self_consistent_field_cycle scf:1292-1435,
// calculate_DIIS_error scf:879-949, apply_DIIS scf:960-1061, apply_damping scf:763-868,
// diagonalise_Fock_matrix scf:222-250, construct_density_matrix scf:183-211,
// calculate_restricted_electronic_energy scf:344-404, calculate_orthogonalisation_matrix kernel:756-816.
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/tunafock.h"
#include "tf_jacobi.hip.h"
#include "tf_refine.hip.h"
#include "tf_eigh_plan.h"  // the eigensolver's layouts, the words of d_scal, the owner of its blocks and its state; no HIP
#include "tf_scf_host.h"   // the host arithmetic of an iteration: small_solve, DiisHistory, damping_factor_tail, scf_converged

namespace tfscf {

// The stream the SCF code of the calling host thread works on: the legacy default stream, except inside a lockstep batch
// (tf_scf_rhf_batch), where every cycle runs on a host thread and a non-blocking stream of its own so that the O(N^3) steps of different
// cycles overlap on the device.
inline thread_local hipStream_t t_stream = nullptr;
#define TFS_ST (tfscf::t_stream)
inline hipError_t tfs_memcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    if (!t_stream) return hipMemcpy(dst, src, bytes, kind);
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, t_stream);
    return e != hipSuccess ? e : hipStreamSynchronize(t_stream);
}
inline hipError_t tfs_sync() { return t_stream ? hipStreamSynchronize(t_stream) : hipDeviceSynchronize(); }

// what the eigensolver's blocks are made of: plain hipMalloc (no allocation cache) and pinned host memory
inline int eig_dev_alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
inline void eig_dev_free(void *p) { (void)hipFree(p); }
inline int eig_pin_alloc(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline void eig_pin_free(void *p) { (void)hipHostFree(p); }

struct Workspace {
    // Sharded tensors (world > 1): every rank runs the cycle redundantly on identical data, and a last-bit difference must not let one
    // rank leave the loop (or take another branch) while the others wait in the next all-reduce.  `agree` sums a few per-iteration
    // decision values over the ranks (tf_ranks_host.hip.h: through the registered all-reduce) and fails on EVERY rank when they differ.
    std::function<int(const double *vals, int n, std::string &msg)> agree;
    rocblas_handle blas = nullptr;
    int n = 0;
    double *pool = nullptr;      // all N x N device matrices live in one allocation
    size_t pool_doubles = 0;
    double *d_scal = nullptr;    // small device scalar array
    double *d_part = nullptr;    // [256][8] block partials of the two-stage reductions
    rocblas_int *d_info = nullptr;   // four status words: one solver, or the (at most four) blocks of a batched one
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_pin = nullptr;     // recorded behind the refinement's per-step read-back into eig.pin
    std::vector<hipEvent_t> tev;     // timing events, read after the cycle (no synchronisation inside it)
    EigState eig{eig_dev_alloc, eig_dev_free, eig_pin_alloc, eig_pin_free};   // the eigensolver's own state and blocks (tf_eigh_plan.h)
};

inline void release(Workspace &w)
{
    if (w.pool) (void)hipFree(w.pool);
    if (w.d_scal) (void)hipFree(w.d_scal);
    if (w.d_part) (void)hipFree(w.d_part);
    if (w.d_info) (void)hipFree(w.d_info);
    if (w.blas) (void)rocblas_destroy_handle(w.blas);
    if (w.ev0) (void)hipEventDestroy(w.ev0);
    if (w.ev1) (void)hipEventDestroy(w.ev1);
    if (w.ev_pin) (void)hipEventDestroy(w.ev_pin);
    for (hipEvent_t e : w.tev) (void)hipEventDestroy(e);
    w.eig.release();
    w = Workspace();
}

#define TFS_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (call);                                                                         \
        if (_e != hipSuccess) { msg = std::string(#call) + " failed: " + hipGetErrorString(_e); return TF_ENODEVICE; } \
    } while (0)
#define TFS_BLAS(call)                                                                                  \
    do {                                                                                                \
        rocblas_status _s = (call);                                                                     \
        if (_s != rocblas_status_success) { msg = std::string(#call) + " failed (rocBLAS/rocSOLVER status " + std::to_string((int)_s) + ")"; return TF_ELINALG; } \
    } while (0)

inline int ensure(Workspace &w, int n, int n_mats, std::string &msg)
{
    if (!w.blas) {
        TFS_BLAS(rocblas_create_handle(&w.blas));
        TFS_HIP(hipMalloc((void **)&w.d_scal, SC_LEN * sizeof(double)));   // the words of ScalWord (tf_eigh_plan.h)
        TFS_HIP(hipMalloc((void **)&w.d_part, 256 * 8 * sizeof(double)));
        TFS_HIP(hipMalloc((void **)&w.d_info, 4 * sizeof(rocblas_int)));
        TFS_HIP(hipEventCreate(&w.ev0));
        TFS_HIP(hipEventCreate(&w.ev1));
    }
    const size_t need = (size_t)n_mats * n * n + 4 * (size_t)n;
    if (need > w.pool_doubles) {
        if (w.pool) (void)hipFree(w.pool);
        w.pool = nullptr; w.pool_doubles = 0;
        TFS_HIP(hipMalloc((void **)&w.pool, need * sizeof(double)));
        w.pool_doubles = need;
    }
    w.n = n;
    return TF_OK;
}

// ---- small element-wise kernels -------------------------------------------------------------------

__global__ void k_symmetrise(const double *__restrict__ in, double *__restrict__ out, int n)   // tuna_util.py:762
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int i = e / n, j = e - i * n;
    out[e] = (1.0 / 2.0) * (in[e] + in[(size_t)j * n + i]);
}

// F = H + J - 1/2 * hfx * K   (scf:525), then symmetrised by k_symmetrise
__global__ void k_fock(const double *__restrict__ H, const double *__restrict__ J, const double *__restrict__ K, double hfx,
                       double *__restrict__ F, int nn)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nn) F[e] = H[e] + J[e] - (1.0 / 2.0) * K[e] * hfx;
}

__global__ void k_axpby(double a, const double *__restrict__ x, double b, const double *__restrict__ y, double *__restrict__ out, int nn)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nn) out[e] = a * x[e] + b * y[e];
}

__global__ void k_scale_cols(const double *__restrict__ V, const double *__restrict__ s, int mode, double *__restrict__ out, int n)
{
    // out[i][k] = V[i][k] * f(s[k]);  mode 0: s^-1/2, mode 1: 1/s     (row-major V, eigenvector k in column k)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int k = e % n;
    out[e] = V[e] * (mode == 0 ? 1.0 / sqrt(s[k]) : 1.0 / s[k]);
}

struct Ptr8 { const double *p[8]; double c[8]; };
#define TF_MAX_DIIS 64           // history entries the native cycles hold (the reference keeps any `DIIS n`, scf:943-946; 8 per launch here)
static_assert(TF_MAX_DIIS == SC_HIST_SPIN, "d_scal holds one history's scalar products per spin");
__global__ void k_lincomb(Ptr8 a, int m, double *__restrict__ out, int nn, int accumulate)     // F_DIIS = sum_k c_k F_k (scf:1025)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nn) return;
    double s = accumulate ? out[e] : 0.0;
    for (int k = 0; k < m; ++k) s += a.c[k] * a.p[k][e];
    out[e] = s;
}

// out[k] = <x, a.p[k]> for k < m (m <= 8): all the scalar products of one SCF step in one launch and one read-back instead of one
// synchronising rocblas_ddot each (at N = 60 the cycle is bound by such round trips).  Single block, fixed summation tree.
__global__ void k_multi_dot(const double *__restrict__ x, Ptr8 a, int m, int nn, double *__restrict__ out)
{
    __shared__ double sm[8][256];
    double acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0;
    for (int e = threadIdx.x; e < nn; e += 256) {
        const double xv = x[e];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < m) acc[k] += xv * a.p[k][e];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sm[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st)
#pragma unroll
            for (int k = 0; k < 8; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < m) out[threadIdx.x] = sm[threadIdx.x][0];
}

// The same in two stages for long vectors (one block over 160 000 elements took 1.1 ms at N = 400, twice per SCF iteration):
// block b leaves its partial sums in part[b][0..7]; k_multi_dot_fin adds the blocks in index order (fixed: reproducible).
__global__ __launch_bounds__(256) void k_multi_dot_part(const double *__restrict__ x, Ptr8 a, int m, int nn, double *__restrict__ part)
{
    __shared__ double sm[8][256];
    double acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0;
    const int per = (nn + gridDim.x - 1) / gridDim.x, e0 = blockIdx.x * per, e1 = min(nn, e0 + per);
    for (int e = e0 + threadIdx.x; e < e1; e += 256) {
        const double xv = x[e];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < m) acc[k] += xv * a.p[k][e];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sm[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st)
#pragma unroll
            for (int k = 0; k < 8; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 8) part[blockIdx.x * 8 + threadIdx.x] = sm[threadIdx.x][0];
}
__global__ void k_multi_dot_fin(const double *__restrict__ part, int nblk, int m, double *__restrict__ out)
{
    const int k = threadIdx.x;
    if (k >= m) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[b * 8 + k];
    out[k] = s;
}

// res[0] = max |a-b|, res[1] = sum (a-b)^2 in two stages (as above)
__global__ __launch_bounds__(256) void k_delta_norms_part(const double *__restrict__ a, const double *__restrict__ b, int nn, double *__restrict__ part)
{
    __shared__ double smax[256], ssum[256];
    double mx = 0.0, sm = 0.0;
    const int per = (nn + gridDim.x - 1) / gridDim.x, e0 = blockIdx.x * per, e1 = min(nn, e0 + per);
    for (int e = e0 + threadIdx.x; e < e1; e += 256) {
        const double d = a[e] - b[e];
        mx = fmax(mx, fabs(d));
        sm += d * d;
    }
    smax[threadIdx.x] = mx; ssum[threadIdx.x] = sm;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]); ssum[threadIdx.x] += ssum[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blockIdx.x * 8] = smax[0]; part[blockIdx.x * 8 + 1] = ssum[0]; }
}
__global__ void k_delta_norms_fin(const double *__restrict__ part, int nblk, double *__restrict__ res)
{
    if (threadIdx.x != 0) return;
    double mx = 0.0, sm = 0.0;
    for (int b = 0; b < nblk; ++b) { mx = fmax(mx, part[b * 8]); sm += part[b * 8 + 1]; }
    res[0] = mx; res[1] = sm;
}

// res[0] = max |a-b|, res[1] = sum (a-b)^2       (scf:285-286), single block
__global__ void k_delta_norms(const double *__restrict__ a, const double *__restrict__ b, int nn, double *__restrict__ res)
{
    __shared__ double smax[256], ssum[256];
    double mx = 0.0, sm = 0.0;
    for (int e = threadIdx.x; e < nn; e += 256) {
        const double d = a[e] - b[e];
        mx = fmax(mx, fabs(d));
        sm += d * d;
    }
    smax[threadIdx.x] = mx; ssum[threadIdx.x] = sm;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]); ssum[threadIdx.x] += ssum[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { res[0] = smax[0]; res[1] = ssum[0]; }
}

// Mulliken gross atomic populations: res[a] = sum_{i in atom a} (P S)_ii   (scf:789-818), single block
__global__ void k_mulliken(const double *__restrict__ P, const double *__restrict__ S, int n, int nA, double *__restrict__ res)
{
    __shared__ double s0[256], s1[256];
    double a0 = 0.0, a1 = 0.0;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        const double v = P[e] * S[(size_t)j * n + i];
        if (i < nA) a0 += v; else a1 += v;
    }
    s0[threadIdx.x] = a0; s1[threadIdx.x] = a1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s0[threadIdx.x] += s0[threadIdx.x + s]; s1[threadIdx.x] += s1[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { res[0] = s0[0]; res[1] = s1[0]; }
}

// row-major C = alpha * op(A) * op(B) + beta * C, all n x n (k = inner dimension, default n)
inline void launch_multi_dot(Workspace &w, const double *x, const Ptr8 &a, int m, int nn, double *out)
{
    if (nn <= 8192) { hipLaunchKernelGGL(k_multi_dot, dim3(1), dim3(256), 0, TFS_ST, x, a, m, nn, out); return; }
    const int nblk = std::min(256, (nn + 2047) / 2048);
    hipLaunchKernelGGL(k_multi_dot_part, dim3(nblk), dim3(256), 0, TFS_ST, x, a, m, nn, w.d_part);
    hipLaunchKernelGGL(k_multi_dot_fin, dim3(1), dim3(64), 0, TFS_ST, w.d_part, nblk, m, out);
}
inline void launch_delta_norms(Workspace &w, const double *a, const double *b, int nn, double *res)
{
    if (nn <= 8192) { hipLaunchKernelGGL(k_delta_norms, dim3(1), dim3(256), 0, TFS_ST, a, b, nn, res); return; }
    const int nblk = std::min(256, (nn + 2047) / 2048);
    hipLaunchKernelGGL(k_delta_norms_part, dim3(nblk), dim3(256), 0, TFS_ST, a, b, nn, w.d_part);
    hipLaunchKernelGGL(k_delta_norms_fin, dim3(1), dim3(64), 0, TFS_ST, w.d_part, nblk, res);
}

inline rocblas_status gemm_rm(rocblas_handle h, bool tA, bool tB, int n, double alpha, const double *A, const double *B, double beta,
                              double *C)
{
    return rocblas_dgemm(h, tB ? rocblas_operation_transpose : rocblas_operation_none,
                         tA ? rocblas_operation_transpose : rocblas_operation_none, n, n, n, &alpha, B, n, A, n, &beta, C, n);
}

#include "tf_eigh.hip.h"   // the symmetric eigensolver, its refinement, orthogonaliser / diagonalise, eigh_probe

using JKFn = std::function<int(const double *, double *, double *, hipStream_t)>;
// Kohn-Sham hook: V_XC (device [N,N]) and {n_elec, E_X, E_C} for the device density (tf_dft.hip.h); empty for Hartree-Fock
using XCFn = std::function<int(const double *, double *, double *)>;

// ---- the stages run_rhf and run_uhf share ---------------------------------------------------------------------
// Each stage queues, on TFS_ST and in this order, the device work its text queued when it stood in both cycles.

// device-time spans without synchronising inside the cycle: events from a pool, read after the last iteration
struct SpanTimer {
    Workspace &w;
    size_t used = 0;
    std::vector<std::pair<size_t, int>> spans;                    // (first event index, 0 = Fock build, 1 = eigensolver)
    int begin(int kind)
    {
        while (w.tev.size() < used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return -1;
            w.tev.push_back(e);
        }
        spans.emplace_back(used, kind);
        (void)hipEventRecord(w.tev[used], TFS_ST);
        used += 2;
        return (int)used - 1;
    }
    void end(int idx) { if (idx >= 0) (void)hipEventRecord(w.tev[idx], TFS_ST); }
    void read(tf_scf_result &out) const                           // after a synchronisation
    {
        for (const auto &sp : spans) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, w.tev[sp.first], w.tev[sp.first + 1]) == hipSuccess) (sp.second == 0 ? out.fock_seconds : out.eig_seconds) += ms * 1e-3;
        }
    }
};

// What the two cycles hold alike: the sizes, the matrices every stage works on (each cycle's own mat(k)), the span timer
struct CycleBase {
    Workspace &w;
    int n; size_t nn; int g;                                      // g: blocks of 256 threads over nn elements
    double *dS, *dH, *dX, *dT, *dV, *dFx, *t1, *t2, *dW, *dC, *scr, *vals, *ework;
    SpanTimer spans;
};

// One matrix of every history entry: logical entry k at base + slot * stride (DiisHistory, tf_scf_host.h)
struct HistMats {
    const DiisHistory &H;
    double *base;
    size_t stride;
    double *operator()(int k) const { return base + (size_t)H.slot_of(k) * stride; }
};

// Prologue, in three steps around the upload of the cycle's own guess densities: S, T, V and the field term; H = T + V (+ field);
// X from the host or from S
inline int upload_integrals(CycleBase &c, const double *S, const double *T, const double *V, const double *Fext, std::string &msg)
{
    TFS_HIP(tfs_memcpy(c.dS, S, c.nn * sizeof(double), hipMemcpyHostToDevice));
    TFS_HIP(tfs_memcpy(c.dT, T, c.nn * sizeof(double), hipMemcpyHostToDevice));
    TFS_HIP(tfs_memcpy(c.dV, V, c.nn * sizeof(double), hipMemcpyHostToDevice));
    if (Fext) TFS_HIP(tfs_memcpy(c.dFx, Fext, c.nn * sizeof(double), hipMemcpyHostToDevice));
    else TFS_HIP(hipMemsetAsync(c.dFx, 0, c.nn * sizeof(double), TFS_ST));
    return TF_OK;
}
inline void core_hamiltonian(CycleBase &c)
{
    hipLaunchKernelGGL(k_axpby, dim3(c.g), dim3(256), 0, TFS_ST, 1.0, c.dT, 1.0, c.dV, c.dH, (int)c.nn);      // H = T + V (+ field)
    hipLaunchKernelGGL(k_axpby, dim3(c.g), dim3(256), 0, TFS_ST, 1.0, c.dH, 1.0, c.dFx, c.dH, (int)c.nn);
}
inline int take_orthogonaliser(CycleBase &c, const double *X, double *scratch, std::string &msg)
{
    double sm = 0;
    if (!X) return orthogonaliser_device(c.w, c.n, c.dS, c.dX, nullptr, &sm, scratch, msg);
    TFS_HIP(tfs_memcpy(c.dX, X, c.nn * sizeof(double), hipMemcpyHostToDevice));
    return TF_OK;
}

// dW = sym(X^T F X)
inline int fock_to_orthogonal(CycleBase &c, const double *Fao, std::string &msg)
{
    TFS_BLAS(gemm_rm(c.w.blas, true, false, c.n, 1.0, c.dX, Fao, 0.0, c.t1));     // X^T F
    TFS_BLAS(gemm_rm(c.w.blas, false, false, c.n, 1.0, c.t1, c.dX, 0.0, c.t2));   // (X^T F) X
    hipLaunchKernelGGL(k_symmetrise, dim3(c.g), dim3(256), 0, TFS_ST, c.t2, c.dW, c.n);
    return TF_OK;
}

// F = sym(H + J - hfx/2 K (+ V_XC))   (scf:497-531, 542-589)
inline void assemble_fock(CycleBase &c, const double *dJ, const double *dK, double hfx, const double *dVxc, double *dF)
{
    hipLaunchKernelGGL(k_fock, dim3(c.g), dim3(256), 0, TFS_ST, c.dH, dJ, dK, hfx, c.t1, (int)c.nn);
    if (dVxc) hipLaunchKernelGGL(k_axpby, dim3(c.g), dim3(256), 0, TFS_ST, 1.0, c.t1, 1.0, dVxc, c.t1, (int)c.nn);        // + V_XC, scf:525
    hipLaunchKernelGGL(k_symmetrise, dim3(c.g), dim3(256), 0, TFS_ST, c.t1, dF, c.n);
}

// DIIS error e = X^T (F P S - S P F) X into histE, F into histF   (scf:906-920)
inline int diis_error(CycleBase &c, const double *dF, const double *dP, double *histE, double *histF, std::string &msg)
{
    rocblas_handle h = c.w.blas;
    const int n = c.n;
    TFS_BLAS(gemm_rm(h, false, false, n, 1.0, dF, dP, 0.0, c.t1));          // F P
    TFS_BLAS(gemm_rm(h, false, false, n, 1.0, c.t1, c.dS, 0.0, c.t2));      // F P S
    TFS_BLAS(gemm_rm(h, false, false, n, 1.0, c.dS, dP, 0.0, c.t1));        // S P
    TFS_BLAS(gemm_rm(h, false, false, n, -1.0, c.t1, dF, 1.0, c.t2));       // F P S - S P F
    TFS_BLAS(gemm_rm(h, true, false, n, 1.0, c.dX, c.t2, 0.0, c.t1));       // X^T e
    TFS_BLAS(gemm_rm(h, false, false, n, 1.0, c.t1, c.dX, 0.0, histE));     // (X^T e) X
    TFS_HIP(hipMemcpyAsync(histF, dF, c.nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
    return TF_OK;
}

// <e_k, e_newest> for every entry of the history into out[k], eight scalar products per launch
inline void history_dots(CycleBase &c, const HistMats &histE, double *out)
{
    const int n_hist = histE.H.n_hist;
    for (int k0 = 0; k0 < n_hist; k0 += 8) {
        Ptr8 a;
        const int mk = std::min(8, n_hist - k0);
        for (int k = 0; k < 8; ++k) { a.p[k] = histE(0); a.c[k] = 0.0; }
        for (int k = 0; k < mk; ++k) a.p[k] = histE(k0 + k);
        launch_multi_dot(c.w, histE(n_hist - 1), a, mk, (int)c.nn, out + k0);
    }
}

// <P, T>, <P, V>, <P, field>, <P, J>, <P, K> into out[0..4]: read back at the end of the iteration, together with the density changes
inline void energy_dots(CycleBase &c, const double *dPn, const double *dJ, const double *dK, double *out)
{
    Ptr8 a;
    for (int k = 0; k < 8; ++k) { a.p[k] = c.dT; a.c[k] = 0.0; }
    a.p[0] = c.dT; a.p[1] = c.dV; a.p[2] = c.dFx; a.p[3] = dJ; a.p[4] = dK;
    launch_multi_dot(c.w, dPn, a, 5, (int)c.nn, out);
}

// scr = sum_k x_k F_k   (scf:1025)
inline void extrapolate_fock(CycleBase &c, const HistMats &histF, const std::vector<double> &x)
{
    const int n_hist = histF.H.n_hist;
    for (int k0 = 0; k0 < n_hist; k0 += 8) {
        Ptr8 a;
        const int mk = std::min(8, n_hist - k0);
        for (int k = 0; k < 8; ++k) { a.p[k] = histF(0); a.c[k] = 0.0; }
        for (int k = 0; k < mk; ++k) { a.p[k] = histF(k0 + k); a.c[k] = x[k0 + k]; }
        hipLaunchKernelGGL(k_lincomb, dim3(c.g), dim3(256), 0, TFS_ST, a, mk, c.scr, (int)c.nn, k0 > 0 ? 1 : 0);
    }
}

// diagonalise F (AO) -> eps, C ; P = occ C_occ C_occ^T symmetrised      (scf:222-250, 183-211; occ = 2, or 1 per spin: scf:1227-1228)
// After the first solve of a cycle the density comes from refined eigenvectors: GEMM-based for n > 64 (where the eigensolver
// would be rocsolver_dsyevd), one LDS-resident launch for n <= 64 (where it would be the Jacobi kernel).  `current`: vals and dC
// hold the eigenpairs of Fao (a full solve).  TF_REFINE_CHECK (debugging) compares every refined density with a real eigensolve.
inline int density_from_fock(CycleBase &c, int n_occ, double occ, const double *Fao, double *Pout, bool &current, std::string &msg)
{
    Workspace &w = c.w;
    const int n = c.n, g = c.g;
    double *t1 = c.t1, *t2 = c.t2, *dW = c.dW, *dC = c.dC;
    static const bool no_refine = getenv("TF_EIGH") != nullptr;
    static const bool no_fused = getenv("TF_REFINE_UNFUSED") != nullptr;
    const bool refining = !no_refine && n >= 2 && n_occ > 0 && n_occ < n;
    const double zero = 0.0;
    current = false;
    if (refining && !no_fused && n <= TFR_NMAX && w.eig.sv().ref_n == n && !getenv("TF_REFINE_CHECK")) {
        const int te = c.spans.begin(1);
        std::string rmsg;
        const int rr = ref_density_lds(w, n, n_occ, Fao, c.dX, Pout, occ, rmsg);
        c.spans.end(te);
        if (rr == TF_OK) return TF_OK;
        if (rr != TF_ELINALG) { msg = rmsg; return rr; }
    }
    int r = fock_to_orthogonal(c, Fao, msg);
    if (r) return r;
    const int te = c.spans.begin(1);
    if (refining && w.eig.sv().ref_n == n) {
        double *Xocc = nullptr;
        std::string rmsg;
        const int rr = (n <= TFR_NMAX) ? ref_refine_lds(w, n, n_occ, dW, &Xocc, rmsg)
                     : (w.eig.sv().blk_n == n) ? ref_refine_blocks(w, n, dW, &Xocc, rmsg) : ref_refine(w, n, n_occ, dW, &Xocc, rmsg);
        if (rr == TF_OK) {
            TFS_BLAS(gemm_rm(w.blas, false, true, n, 1.0, Xocc, c.dX, 0.0, t1));    // rows: occupied orbitals in the AO basis (others 0)
            TFS_BLAS(rocblas_dgemm(w.blas, rocblas_operation_none, rocblas_operation_transpose, n, n, n, &occ, t1, n, t1, n, &zero, t2, n));
            hipLaunchKernelGGL(k_symmetrise, dim3(g), dim3(256), 0, TFS_ST, t2, Pout, n);
            c.spans.end(te);
            if (getenv("TF_REFINE_CHECK")) {                 // debugging aid: the same density from a real eigensolve
                std::vector<double> hp(c.nn), hq(c.nn);
                TFS_HIP(tfs_memcpy(hp.data(), Pout, c.nn * sizeof(double), hipMemcpyDeviceToHost));
                int r2 = eigh(w, n, dW, c.vals, c.ework, msg);
                if (r2) return r2;
                TFS_BLAS(gemm_rm(w.blas, false, true, n, 1.0, c.dX, dW, 0.0, dC));
                TFS_BLAS(rocblas_dgemm(w.blas, rocblas_operation_transpose, rocblas_operation_none, n, n, n_occ, &occ, dC, n, dC, n, &zero, t1, n));
                hipLaunchKernelGGL(k_symmetrise, dim3(g), dim3(256), 0, TFS_ST, t1, t2, n);
                TFS_HIP(tfs_memcpy(hq.data(), t2, c.nn * sizeof(double), hipMemcpyDeviceToHost));
                double dmax = 0.0;
                for (size_t q = 0; q < c.nn; ++q) dmax = std::max(dmax, std::fabs(hp[q] - hq[q]));
                fprintf(stderr, "[tf refine] max |P_refined - P_eigh| = %.3e\n", dmax);
            }
            return TF_OK;
        }
        if (rr != TF_ELINALG) { msg = rmsg; return rr; }
    }
    r = eigh(w, n, dW, c.vals, c.ework, msg);
    if (r) return r;
    if (refining) { r = ref_store(w, n, dW, msg, n_occ); if (r) return r; }
    c.spans.end(te);
    TFS_BLAS(gemm_rm(w.blas, false, true, n, 1.0, c.dX, dW, 0.0, dC));      // C = X V   (dW rows = eigenvectors)
    // col-major view of dC is C^T: P = sum_{k<nocc} C[:,k] C[:,k]^T = M[:nocc,:]^T M[:nocc,:]
    TFS_BLAS(rocblas_dgemm(w.blas, rocblas_operation_transpose, rocblas_operation_none, n, n, n_occ, &occ, dC, n, dC, n, &zero, t1, n));
    hipLaunchKernelGGL(k_symmetrise, dim3(g), dim3(256), 0, TFS_ST, t1, Pout, n);
    current = true;
    return TF_OK;
}

// orbitals and orbital energies of a cycle's last Fock matrix, when its last density did not come from a full solve of it
// (what the reference's last diagonalisation leaves, scf:1133, 1224-1225)
inline int final_orbitals(CycleBase &c, const double *dF, double *eps, double *C, std::string &msg)
{
    int rc = fock_to_orthogonal(c, dF, msg);
    if (rc) return rc;
    const int te = c.spans.begin(1);
    rc = eigh(c.w, c.n, c.dW, c.vals, c.ework, msg);
    if (rc) return rc;
    TFS_BLAS(gemm_rm(c.w.blas, false, true, c.n, 1.0, c.dX, c.dW, 0.0, c.dC));
    c.spans.end(te);
    if (eps) TFS_HIP(tfs_memcpy(eps, c.vals, c.n * sizeof(double), hipMemcpyDeviceToHost));
    if (C) TFS_HIP(tfs_memcpy(C, c.dC, c.nn * sizeof(double), hipMemcpyDeviceToHost));
    return TF_OK;
}

// The table row of an iteration, its convergence test (scf:261-333), and the agreement of the ranks on both
inline int report_iteration(Workspace &w, const tf_scf_opts &o, tf_scf_result &out, int step, int n_hist, double E_total, double dE,
                            double rmsDP, double maxDP, double commutator, double damp, std::string &msg)
{
    out.n_iter = step;
    if (out.table) {
        double *row = out.table + (size_t)(step - 1) * 7;
        row[0] = step; row[1] = E_total; row[2] = dE; row[3] = rmsDP; row[4] = maxDP; row[5] = commutator; row[6] = damp;
    }
    const bool conv_now = scf_converged(o, dE, maxDP, rmsDP, commutator);
    if (w.agree) {                                               // collective control flow on a sharded tensor
        const double vals[3] = {conv_now ? 1.0 : 0.0, (double)n_hist, (double)step};
        int rc = w.agree(vals, 3, msg);
        if (rc) return rc;
    }
    out.converged = conv_now;
    return TF_OK;
}

// Epilogue, after the last synchronisation and the copies of the cycle's own matrices
inline int finish_cycle(const CycleBase &c, const tf_scf_opts &o, tf_scf_result &out, double E_total, const double comps[7],
                        std::chrono::steady_clock::time_point t_wall, std::string &msg)
{
    c.spans.read(out);
    out.energy = E_total;
    std::memcpy(out.components, comps, 7 * sizeof(double));
    out.wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wall).count();
    if (!out.converged) { msg = "Self-consistent field not converged in " + std::to_string(o.max_iter) + " iterations! Increase maximum iterations or give up."; return TF_ENOTCONV; }
    return TF_OK;
}

// world > 1: the J/K hook completes the partial sums of this rank's tensor rows with the communicator (tf_comm_init) or the registered
// all-reduce (tf_set_allreduce); every rank then runs the O(N^3) steps redundantly on identical data
inline int run_rhf(Workspace &w, int n, const tf_scf_opts &o, const double *S, const double *T, const double *V, const double *Fext,
                   const double *X, const double *P0, double E0, int n_occ, double V_NN, const JKFn &jk,
                   tf_scf_result &out, std::string &msg, const XCFn &xc = XCFn())
{
    if (o.max_diis > TF_MAX_DIIS) { msg = "tf_scf_rhf: at most 64 DIIS matrices are held by the native cycle"; return TF_EINVAL; }
    const int max_diis = std::max(1, (int)o.max_diis);
    const int n_mats = 22 + 2 * max_diis;
    int rc = ensure(w, n, n_mats, msg);
    if (rc) return rc;
    TFS_BLAS(rocblas_set_stream(w.blas, TFS_ST));
    const size_t nn = (size_t)n * n;
    const int g = (int)((nn + 255) / 256);
    auto t_wall = std::chrono::steady_clock::now();
    double *base = w.pool;
    auto mat = [&](int k) { return base + (size_t)k * nn; };
    double *dS = mat(0), *dH = mat(1), *dX = mat(2), *dP = mat(3), *dPold = mat(4), *dPbd = mat(5), *dPvold = mat(6), *dPoldbd = mat(7);
    double *dF = mat(8), *dJ = mat(9), *dK = mat(10), *dT = mat(11), *dV = mat(12), *dFx = mat(13), *t1 = mat(14), *t2 = mat(15);
    double *dC = mat(16), *dW = mat(17), *dPn = mat(18), *scr = mat(19), *dVxc = mat(20), *dCsave = mat(21);
    double *hist = mat(22);
    double *vals = base + (size_t)n_mats * nn, *ework = vals + n, *vals_save = ework + n;
    CycleBase c{w, n, nn, g, dS, dH, dX, dT, dV, dFx, t1, t2, dW, dC, scr, vals, ework, SpanTimer{w}};
    DiisHistory H(max_diis);
    const HistMats histF{H, hist, 2 * nn}, histE{H, hist + nn, 2 * nn};

    rc = upload_integrals(c, S, T, V, Fext, msg);
    if (rc) return rc;
    TFS_HIP(tfs_memcpy(dP, P0, nn * sizeof(double), hipMemcpyHostToDevice));
    core_hamiltonian(c);
    rc = take_orthogonaliser(c, X, scr, msg);
    if (rc) return rc;
    for (double *zeroed : {dPold, dPbd, dPvold, dPoldbd}) TFS_HIP(hipMemsetAsync(zeroed, 0, nn * sizeof(double), TFS_ST));
    TFS_BLAS(rocblas_set_pointer_mode(w.blas, rocblas_pointer_mode_host));
    bool orbitals_current = false, orbitals_final = false;
    EigState &eg = w.eig;
    eg.forget_vectors();
    eg.warm_ok = true;                // successive Fock matrices are close: warm-start the Jacobi solver from the last eigenvectors
    eg.jac_prev_n = 0; eg.sym_prev_n = 0; // (no warm start across cycles: a cycle's result must not depend on what the context solved before)
    struct WarmGuard { EigState &e; ~WarmGuard() { e.warm_ok = false; e.jac_prev_n = 0; e.sym_prev_n = 0; e.eig_fail = nullptr; } } warm_guard{eg};
    eg.eig_fail = w.d_scal + SC_FAIL_RHF; // solver status of the iteration, read back with its density changes
    TFS_HIP(hipMemsetAsync(eg.eig_fail, 0, sizeof(double), TFS_ST));
    double E = E0, E_old = E0, commutator = 1.0;
    double comps[7] = {0, 0, 0, 0, 0, 0, 0};
    out.fock_seconds = 0; out.eig_seconds = 0; out.n_iter = 0; out.converged = 0;
    const int nA = (o.n_atoms >= 2) ? o.n_atom_ao[0] : n;

    for (int step = 1; step <= o.max_iter; ++step) {
        E_old = E;
        // P_very_old = P_old ; P_old = P    (scf:1114-1117).  "P_old_before_damping" is the zero matrix in every
        // iteration of the reference: run_restricted_SCF_cycle does not return P_before_damping (scf:1154), so the
        // outer loop keeps handing in its initial zeros (scf:1359,1373).  dPoldbd therefore stays zero.
        std::swap(dPvold, dPold);            // dPvold <- old P_old ; dPold free to be overwritten
        TFS_HIP(hipMemcpyAsync(dPold, dP, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
        // Fock matrix (scf:497-531)
        // Kohn-Sham: exchange-correlation matrix and energy densities from the CURRENT (old) density (scf:1121)
        double xc3[3] = {0.0, 0.0, 0.0};
        if (xc) {
            rc = xc(dP, dVxc, xc3);
            if (rc) { msg = "exchange-correlation evaluation failed"; return rc; }
        }
        const int tf = c.spans.begin(0);
        rc = jk(dP, dJ, dK, TFS_ST);
        if (rc) { msg.clear(); return rc; }                          // (the hook has left its message in the context)
        c.spans.end(tf);
        H.make_room();                                               // before the push, so that the slot of the new entry is known
        static const bool no_fused_fock = getenv("TF_FOCK_UNFUSED") != nullptr;
        hipError_t ferr = hipSuccess;
        if (!no_fused_fock && n <= TFR_NMAX &&
            tfref::launch_fock_diis(n, dH, dJ, dK, o.hfx, xc ? dVxc : nullptr, dP, dS, dX, dF, histF(H.n_hist), histE(H.n_hist), TFS_ST, &ferr)) {
            // n <= 64: Fock matrix, DIIS error and the history entry in one launch (tf_refine.hip.h)
        } else {
            if (ferr != hipSuccess) { msg = std::string("Fock / DIIS kernel launch failed: ") + hipGetErrorString(ferr); return TF_ENODEVICE; }
            assemble_fock(c, dJ, dK, o.hfx, xc ? dVxc : nullptr, dF);
            rc = diis_error(c, dF, dP, histE(H.n_hist), histF(H.n_hist), msg);
            if (rc) return rc;
        }
        ++H.n_hist;
        double hd[TF_MAX_DIIS], row[TF_MAX_DIIS];
        history_dots(c, histE, w.d_scal + SC_HIST);
        TFS_HIP(tfs_memcpy(hd, w.d_scal + SC_HIST, H.n_hist * sizeof(double), hipMemcpyDeviceToHost));
        // the reference stores the error twice (alpha and beta copies, scf:934), hence the factor 2
        for (int k = 0; k < H.n_hist; ++k) row[k] = 2.0 * hd[k];
        H.enter_dots(row);
        commutator = std::sqrt(hd[H.n_hist - 1] / (double)nn);                         // scf:918
        // diagonalise, new density, energy with the NEW P and the OLD J,K   (scf:1133-1141)
        rc = density_from_fock(c, n_occ, 2.0, dF, dPn, orbitals_current, msg);
        if (rc) return rc;
        energy_dots(c, dPn, dJ, dK, w.d_scal + SC_ENERGY);
        orbitals_final = orbitals_current;                            // of THIS iteration's Fock matrix (the DIIS solve below reuses dC)
        if (orbitals_final && (out.eps || out.C)) {                  // kept on the device; copied out after the cycle
            TFS_HIP(hipMemcpyAsync(vals_save, vals, n * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
            TFS_HIP(hipMemcpyAsync(dCsave, dC, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
        }
        // DIIS extrapolation (scf:991-1059)
        double *Pcur = dPn;
        std::vector<double> x;
        if (step > 2 && o.use_diis && commutator < 0.3 && H.solve(x)) {
            extrapolate_fock(c, histF, x);
            rc = density_from_fock(c, n_occ, 2.0, scr, dPn, orbitals_current, msg);     // overwrites dC/vals: results were copied out above
            if (rc) return rc;
        }
        // P_before_damping = P ; damping (scf:763-868)
        TFS_HIP(hipMemcpyAsync(dPbd, Pcur, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
        double damp = 0.0;
        if (o.damping == 2) damp = o.damping_factor;
        else if (o.damping == 1 && commutator > 0.01 && step > 1) {
            double pop[4][2];
            const double *dens[4] = {dPbd, dPold, dPoldbd, dPvold};   // A_n_out, A_n1_in, A_n1_out, A_n2_in
            for (int q = 0; q < 4; ++q) hipLaunchKernelGGL(k_mulliken, dim3(1), dim3(256), 0, TFS_ST, dens[q], dS, n, nA, w.d_scal + SC_POP + 2 * q);
            TFS_HIP(tfs_memcpy(&pop[0][0], w.d_scal + SC_POP, SC_POP_LEN * sizeof(double), hipMemcpyDeviceToHost));
            if (o.n_atoms < 2) { for (int q = 0; q < 4; ++q) pop[q][1] = 0.0; }
            double num[2], den[2];
            for (int a = 0; a < 2; ++a) { num[a] = pop[0][a] - pop[2][a]; den[a] = pop[0][a] - pop[2][a] - pop[1][a] + pop[3][a]; }
            damp = damping_factor_tail(o, num, den);
        }
        hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, TFS_ST, damp, dPold, 1.0 - damp, dPbd, dP, (int)nn);
        // changes and convergence (scf:261-333)
        launch_delta_norms(w, dP, dPold, (int)nn, w.d_scal + SC_DELTA);
        double res[8];
        TFS_HIP(tfs_memcpy(res, w.d_scal + SC_DELTA, 8 * sizeof(double), hipMemcpyDeviceToHost));   // ... SC_FAIL_RHF
        if (res[7] != 0.0) { msg = "Eigenvalues did not converge (SCF iteration " + std::to_string(step) + ")"; return TF_ELINALG; }
        {
            const double eT = res[2], eV = res[3], eF = res[4], eJ = res[5], eK = res[6];
            comps[0] = eT; comps[1] = eV; comps[2] = (1.0 / 2.0) * eJ; comps[3] = -(1.0 / 4.0) * eK * o.hfx + xc3[1]; comps[4] = xc3[2];   // scf:380-394
            comps[5] = eF; comps[6] = 0.0;
            E = comps[0] + comps[1] + comps[2] + comps[3] + comps[4] + comps[5] + comps[6];
        }
        rc = report_iteration(w, o, out, step, H.n_hist, E + V_NN, E - E_old, std::sqrt(res[1] / (double)nn), res[0], commutator, damp, msg);
        if (rc) return rc;
        if (out.converged) break;
    }
    if (orbitals_final) {
        if (out.eps) TFS_HIP(tfs_memcpy(out.eps, vals_save, n * sizeof(double), hipMemcpyDeviceToHost));
        if (out.C) TFS_HIP(tfs_memcpy(out.C, dCsave, nn * sizeof(double), hipMemcpyDeviceToHost));
    }
    eg.eig_fail = nullptr;
    if (!orbitals_final && (out.eps || out.C) && out.n_iter > 0) {
        rc = final_orbitals(c, dF, out.eps, out.C, msg);
        if (rc) return rc;
    }
    eg.forget_vectors();
    TFS_HIP(tfs_sync());
    if (out.P) TFS_HIP(tfs_memcpy(out.P, dP, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (out.F) TFS_HIP(tfs_memcpy(out.F, dF, nn * sizeof(double), hipMemcpyDeviceToHost));
    return finish_cycle(c, o, out, E + V_NN, comps, t_wall, msg);
}

// ---- unrestricted cycle: run_unrestricted_SCF_cycle (scf:1165-1281) inside the outer loop (scf:1292-1435) ---------------------
// Both spin densities go through the tensor in one fused pass (jk2); every O(N^3) step on the device; per iteration the host reads
// back a handful of scalars (DIIS scalar products, energy terms, populations, density changes).  Reference behaviour kept: the error
// vector of an iteration is the concatenation of the alpha and beta commutators (scf:1213), the commutator reported is the larger
// of the two (scf:1211), each spin is damped with its own factor (scf:1259-1260) in which "P_very_old" and "P_old_before_damping" are
// zero matrices in every iteration (scf:1281 against scf:1394), and the table shows the larger factor.
using JK2Fn = std::function<int(const double *, const double *, double *, double *, double *, double *, hipStream_t)>;

struct UhfOut {
    double *P[2], *C[2], *eps[2], *F[2];                        // host buffers, each may be nullptr
};
// unrestricted Kohn-Sham hook: V_XC^alpha, V_XC^beta (device [N,N]) and {n_alpha, n_beta, E_X,alpha, E_X,beta, E_C} for the device
// densities (tfdft::vxc_unrestricted); empty for Hartree-Fock
using XC2Fn = std::function<int(const double *, const double *, double *, double *, double *)>;

inline int run_uhf(Workspace &w, int n, const tf_scf_opts &o, const double *S, const double *T, const double *V, const double *Fext,
                   const double *X, const double *Pa0, const double *Pb0, double E0, int n_alpha, int n_beta, double V_NN, const JK2Fn &jk2,
                   tf_scf_result &out, const UhfOut &uo, std::string &msg, const XC2Fn &xc = XC2Fn())
{
    if (o.max_diis > TF_MAX_DIIS) { msg = "tf_scf_uhf: at most 64 DIIS matrices are held by the native cycle"; return TF_EINVAL; }
    const int max_diis = std::max(1, (int)o.max_diis);
    const int n_fixed = xc ? 32 : 30;                               // (Kohn-Sham: V_XC^alpha, V_XC^beta in mat(30), mat(31))
    const int n_mats = n_fixed + 4 * max_diis;
    int rc = ensure(w, n, n_mats, msg);
    if (rc) return rc;
    TFS_BLAS(rocblas_set_stream(w.blas, TFS_ST));
    const size_t nn = (size_t)n * n;
    const int g = (int)((nn + 255) / 256);
    auto t_wall = std::chrono::steady_clock::now();
    double *base = w.pool;
    auto mat = [&](int k) { return base + (size_t)k * nn; };
    double *dS = mat(0), *dH = mat(1), *dX = mat(2), *dT = mat(3), *dV = mat(4), *dFx = mat(5), *t1 = mat(6), *t2 = mat(7), *dW = mat(8);
    double *dC = mat(9), *scr = mat(10), *dPt = mat(11), *dPtold = mat(12);
    double *dP[2] = {mat(13), mat(14)}, *dPold[2] = {mat(15), mat(16)}, *dPn[2] = {mat(17), mat(18)}, *dF[2] = {mat(19), mat(20)};
    double *dJ[2] = {mat(21), mat(22)}, *dK[2] = {mat(23), mat(24)}, *dCsave[2] = {mat(25), mat(26)};
    double *dJt = mat(27);                                       // J_alpha + J_beta; mat(28), mat(29): orthogonaliser scratch
    double *dVxc[2] = {xc ? mat(30) : nullptr, xc ? mat(31) : nullptr};
    double *hist = mat(n_fixed);
    double *vals = base + (size_t)n_mats * nn, *ework = vals + n, *vals_save[2] = {ework + n, ework + 2 * (size_t)n};
    CycleBase c{w, n, nn, g, dS, dH, dX, dT, dV, dFx, t1, t2, dW, dC, scr, vals, ework, SpanTimer{w}};
    DiisHistory H(max_diis);                                     // one history for both spins: four matrices per entry
    const HistMats histF[2] = {{H, hist, 4 * nn}, {H, hist + nn, 4 * nn}}, histE[2] = {{H, hist + 2 * nn, 4 * nn}, {H, hist + 3 * nn, 4 * nn}};
    const int n_occ[2] = {n_alpha, n_beta};

    rc = upload_integrals(c, S, T, V, Fext, msg);
    if (rc) return rc;
    TFS_HIP(tfs_memcpy(dP[0], Pa0, nn * sizeof(double), hipMemcpyHostToDevice));
    TFS_HIP(tfs_memcpy(dP[1], Pb0, nn * sizeof(double), hipMemcpyHostToDevice));
    core_hamiltonian(c);
    hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, TFS_ST, 1.0, dP[0], 1.0, dP[1], dPt, (int)nn);
    rc = take_orthogonaliser(c, X, mat(28), msg);
    if (rc) return rc;
    TFS_BLAS(rocblas_set_pointer_mode(w.blas, rocblas_pointer_mode_host));

    // the refinement state of the beta spin is the second SpinVectors of the eigensolver: current around its solves
    EigState &eg = w.eig;
    struct SpinSlot {
        EigState &e; int before;
        SpinSlot(EigState &es, int sp) : e(es), before(es.cur) { e.cur = sp; }
        ~SpinSlot() { e.cur = before; }
    };
    eg.forget_vectors();
    eg.warm_ok = false; eg.jac_prev_n = 0; eg.sym_prev_n = 0;       // two alternating spins: no warm start for the (rare) Jacobi solves
    struct FailGuard { EigState &e; ~FailGuard() { e.eig_fail = nullptr; } } fail_guard{eg};
    eg.eig_fail = w.d_scal + SC_FAIL_UHF; // solver status of the iteration, read back with its density changes
    TFS_HIP(hipMemsetAsync(eg.eig_fail, 0, sizeof(double), TFS_ST));
    bool orbitals_current[2] = {false, false}, orbitals_final[2] = {false, false};
    // diagonalise F_s (AO) -> P_s = C_occ C_occ^T symmetrised (one electron per orbital, scf:1227-1228)
    auto diag_density = [&](int sp, const double *Fao, double *Pout) -> int {
        orbitals_current[sp] = false;
        if (n_occ[sp] <= 0) { TFS_HIP(hipMemsetAsync(Pout, 0, nn * sizeof(double), TFS_ST)); return TF_OK; }
        SpinSlot slot(eg, sp);
        return density_from_fock(c, n_occ[sp], 1.0, Fao, Pout, orbitals_current[sp], msg);
    };

    double E = E0, E_old = E0, commutator = 1.0;
    double comps[7] = {0, 0, 0, 0, 0, 0, 0};
    out.fock_seconds = 0; out.eig_seconds = 0; out.n_iter = 0; out.converged = 0;
    const int nA = (o.n_atoms >= 2) ? o.n_atom_ao[0] : n;

    for (int step = 1; step <= o.max_iter; ++step) {
        E_old = E;
        TFS_HIP(hipMemcpyAsync(dPtold, dPt, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
        for (int sp = 0; sp < 2; ++sp) TFS_HIP(hipMemcpyAsync(dPold[sp], dP[sp], nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
        // Kohn-Sham: exchange-correlation matrices and energies from the iteration's input densities (scf:1237-1240)
        double xc5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (xc) {
            rc = xc(dP[0], dP[1], dVxc[0], dVxc[1], xc5);
            if (rc) { msg = "exchange-correlation evaluation failed"; return rc; }
        }
        // Fock matrices (scf:542-589): F_s = H + J_alpha + J_beta - HFX K_s (+ V_XC^s), symmetrised
        const int tf = c.spans.begin(0);
        rc = jk2(dP[0], dP[1], dJ[0], dJ[1], dK[0], dK[1], TFS_ST);
        if (rc) { msg.clear(); return rc; }
        c.spans.end(tf);
        hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, TFS_ST, 1.0, dJ[0], 1.0, dJ[1], dJt, (int)nn);
        H.make_room();                                              // trim the history to max_diis entries (scf:1216-1219)
        for (int sp = 0; sp < 2; ++sp) {
            assemble_fock(c, dJt, dK[sp], 2.0 * o.hfx, dVxc[sp], dF[sp]);                   // k_fock: H + J - hfx/2 K
            rc = diis_error(c, dF[sp], dP[sp], histE[sp](H.n_hist), histF[sp](H.n_hist), msg);   // e_s = X^T (F_s P_s S - S P_s F_s) X
            if (rc) return rc;
        }
        ++H.n_hist;
        double hd[2 * TF_MAX_DIIS], row[TF_MAX_DIIS];
        for (int sp = 0; sp < 2; ++sp) history_dots(c, histE[sp], w.d_scal + SC_HIST + SC_HIST_SPIN * sp);
        TFS_HIP(tfs_memcpy(hd, w.d_scal + SC_HIST, 2 * TF_MAX_DIIS * sizeof(double), hipMemcpyDeviceToHost));
        for (int k = 0; k < H.n_hist; ++k) row[k] = hd[k] + hd[TF_MAX_DIIS + k];
        H.enter_dots(row);
        const double ee[2] = {hd[H.n_hist - 1], hd[TF_MAX_DIIS + H.n_hist - 1]};
        const double comm_s[2] = {std::sqrt(ee[0] / (double)nn), std::sqrt(ee[1] / (double)nn)};
        commutator = std::max(comm_s[0], comm_s[1]);                  // scf:1211
        // new densities from F_alpha, F_beta; energy with the NEW densities and the OLD J, K (scf:1224-1232)
        for (int sp = 0; sp < 2; ++sp) {
            rc = diag_density(sp, dF[sp], dPn[sp]);
            if (rc) return rc;
            orbitals_final[sp] = orbitals_current[sp];
            if (orbitals_final[sp]) {
                TFS_HIP(hipMemcpyAsync(vals_save[sp], vals, n * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
                TFS_HIP(hipMemcpyAsync(dCsave[sp], dC, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
            }
        }
        for (int sp = 0; sp < 2; ++sp) energy_dots(c, dPn[sp], dJt, dK[sp], w.d_scal + SC_ENERGY + SC_ENERGY_SPIN * sp);
        // DIIS (scf:1236-1256): one set of coefficients for both spins
        std::vector<double> x;
        if (step > 2 && o.use_diis && commutator < 0.3 && H.solve(x)) {
            for (int sp = 0; sp < 2; ++sp) {
                extrapolate_fock(c, histF[sp], x);
                rc = diag_density(sp, scr, dPn[sp]);
                if (rc) return rc;
            }
        }
        // damping, each spin with its own commutator (scf:1259-1260; calculate_damping_factor scf:763-868 with zero
        // "P_very_old" / "P_old_before_damping")
        double damp[2] = {0.0, 0.0};
        if (o.damping == 2) damp[0] = damp[1] = o.damping_factor;
        else if (o.damping == 1 && step > 1 && (comm_s[0] > 0.01 || comm_s[1] > 0.01)) {
            double pop[4][2];
            const double *dens[4] = {dPn[0], dPold[0], dPn[1], dPold[1]};
            for (int q = 0; q < 4; ++q) hipLaunchKernelGGL(k_mulliken, dim3(1), dim3(256), 0, TFS_ST, dens[q], dS, n, nA, w.d_scal + SC_POP + 2 * q);
            TFS_HIP(tfs_memcpy(&pop[0][0], w.d_scal + SC_POP, SC_POP_LEN * sizeof(double), hipMemcpyDeviceToHost));
            if (o.n_atoms < 2) { for (int q = 0; q < 4; ++q) pop[q][1] = 0.0; }
            for (int sp = 0; sp < 2; ++sp) {
                if (!(comm_s[sp] > 0.01)) continue;
                const double *out_p = pop[2 * sp], *in_p = pop[2 * sp + 1];
                const double den[2] = {out_p[0] - in_p[0], out_p[1] - in_p[1]};
                damp[sp] = damping_factor_tail(o, out_p, den);
            }
        }
        for (int sp = 0; sp < 2; ++sp)
            hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, TFS_ST, damp[sp], dPold[sp], 1.0 - damp[sp], dPn[sp], dP[sp], (int)nn);
        hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, TFS_ST, 1.0, dP[0], 1.0, dP[1], dPt, (int)nn);
        launch_delta_norms(w, dPt, dPtold, (int)nn, w.d_scal + SC_DELTA);
        double res[15];
        TFS_HIP(tfs_memcpy(res, w.d_scal + SC_DELTA, 15 * sizeof(double), hipMemcpyDeviceToHost));   // ... SC_FAIL_UHF
        if (res[14] != 0.0) { msg = "Eigenvalues did not converge (SCF iteration " + std::to_string(step) + ")"; return TF_ELINALG; }
        {
            const double *hd = res + 2;
            comps[0] = hd[0] + hd[6]; comps[1] = hd[1] + hd[7]; comps[5] = hd[2] + hd[8];
            comps[2] = (1.0 / 2.0) * (hd[3] + hd[9]);                                        // scf:462
            comps[3] = -(1.0 / 2.0) * hd[4] * o.hfx + -(1.0 / 2.0) * hd[10] * o.hfx;         // scf:465-466
            comps[4] = 0.0; comps[6] = 0.0;
            if (xc) { comps[3] += xc5[2] + xc5[3]; comps[4] = xc5[4]; }                       // scf:467-472
            E = comps[0] + comps[1] + comps[2] + comps[3] + comps[4] + comps[5] + comps[6];
        }
        rc = report_iteration(w, o, out, step, H.n_hist, E + V_NN, E - E_old, std::sqrt(res[1] / (double)nn), res[0], commutator,
                              std::max(damp[0], damp[1]), msg);
        if (rc) return rc;
        if (out.converged) break;
    }
    eg.eig_fail = nullptr;
    // orbitals and orbital energies of the last Fock matrices
    for (int sp = 0; sp < 2 && out.n_iter > 0; ++sp) {
        if (!uo.eps[sp] && !uo.C[sp]) continue;
        if (orbitals_final[sp]) {
            if (uo.eps[sp]) TFS_HIP(tfs_memcpy(uo.eps[sp], vals_save[sp], n * sizeof(double), hipMemcpyDeviceToHost));
            if (uo.C[sp]) TFS_HIP(tfs_memcpy(uo.C[sp], dCsave[sp], nn * sizeof(double), hipMemcpyDeviceToHost));
            continue;
        }
        rc = final_orbitals(c, dF[sp], uo.eps[sp], uo.C[sp], msg);
        if (rc) return rc;
    }
    eg.forget_vectors();
    TFS_HIP(tfs_sync());
    for (int sp = 0; sp < 2; ++sp) {
        if (uo.P[sp]) TFS_HIP(tfs_memcpy(uo.P[sp], dP[sp], nn * sizeof(double), hipMemcpyDeviceToHost));
        if (uo.F[sp]) TFS_HIP(tfs_memcpy(uo.F[sp], dF[sp], nn * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (out.P) TFS_HIP(tfs_memcpy(out.P, dPt, nn * sizeof(double), hipMemcpyDeviceToHost));
    return finish_cycle(c, o, out, E + V_NN, comps, t_wall, msg);
}

}  // namespace tfscf
