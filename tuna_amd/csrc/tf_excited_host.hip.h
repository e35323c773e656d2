// tf_excited_host.hip.h -- the host drivers of the excited states and the stability analysis: CIS / TDHF and TD-DFT / TDA on restricted
// and unrestricted orbitals, the exchange-correlation kernel builds and their probes, RHF / UHF / RKS / UKS stability, and CIS(D).
// Included by tf_device.hip after tf_corr_host.hip.h (one translation unit), whose shared pieces it uses: corr_fail, BlasAtomicsOff,
// CorrSetup, corr_args, corr_begin, mo_transform_device, mo_vvoo_block, mp3_mo_blocks, corr_stamp, corr_secs, corr_stage_seconds; from
// tf_dft_host.hip.h: dft_grid_checks, ensure_spin and the density stages of V_XC (density_stage, density2_stage).  Kernels:
// tf_cis.hip.h, tf_ucis.hip.h, tf_cisd.hip.h, tf_xckernel.hip.h, tf_dft.hip.h; work space: tf_excited_plan.h.  DESIGN.md section 4.5c; the
// invariants of section 4.5a hold here too: every driver keeps its order of launches, rocBLAS / rocSOLVER calls and copies on the null stream.
#pragma once
#include "tf_excited_plan.h"

// ---- CIS / TDHF and the stability analysis: the solve stages tf_cis_rhf and tf_cis_uhf share -------------------------------------

#define CIS_BLAS(call) CORR_BLAS_WHAT("rocBLAS / rocSOLVER", call)

// What a solve stage works with: the driver's names for its messages, the handle, the order of the matrices, the first four sections of
// the plan's small array, and -- TDHF -- the dim^2 array T of the triangular products and the kept vectors Q | Xk | Yk
struct __attribute__((visibility("hidden"))) CisSolve {
    tf_ctx *ctx = nullptr;
    const char *who = "", *ref = "";                          // "tf_cis_rhf", "RHF"
    rocblas_handle blas = nullptr;
    int dim = 0, nk = 0;
    rocblas_int *d_info = nullptr;
    double *d_w = nullptr, *d_w2 = nullptr, *d_e = nullptr, *d_stat = nullptr, *T = nullptr, *Q = nullptr, *Xk = nullptr, *Yk = nullptr;
    bool info(int *h) const { return hipMemcpy(h, d_info, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess; }
    int fail(int code, const std::string &m) const { return corr_fail(ctx, code, std::string(who) + m); }
};

// mu_n[c] = scale sum_ia D^c_ia V[ia][n] over the states (columns) of V, and the oscillator strengths, to the host
static int cis_transition_moments(const CisSolve &s, const ExcitedPlan &P, double *small, const double *V, double scale, double *tdm, double *osc)
{
    const int dim = s.dim;
    double *d_mu = P.at(small, EXC_MU), *d_f = P.at(small, EXC_F);
    int rc = TF_OK;
    if (tfmp3::gemm_rm(s.blas, false, true, dim, 3, dim, scale, V, dim, P.at(small, EXC_DIA), dim, 0.0, d_mu, 3) != rocblas_status_success) rc = TF_ELINALG;
    else {
        hipLaunchKernelGGL(tfcis::oscillator_kernel, dim3((unsigned)((dim + 255) / 256)), dim3(256), 0, 0, d_mu, s.d_w, dim, d_f);
        if ((tdm && hipMemcpy(tdm, d_mu, 3 * (size_t)dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
            (osc && hipMemcpy(osc, d_f, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
            rc = TF_ENODEVICE;
    }
    return rc ? s.fail(rc, ": the transition moments failed on the device") : TF_OK;
}

// A - B = L L^T in place (lower).  Not positive definite: the reference is unstable, TF_ELINALG; whom = " for singlets or triplets" or ""
static int cis_tdhf_factor(const CisSolve &s, double *Mm, const char *whom)
{
    tf_ctx *ctx = s.ctx; const char *who = s.who;
    CIS_BLAS(rocsolver_dpotrf(s.blas, rocblas_fill_lower, s.dim, Mm, s.dim, s.d_info));
    int h = 0;
    if (!s.info(&h)) return s.fail(TF_ENODEVICE, ": the Cholesky factorisation failed on the device");
    if (h != 0) {
        char text[300];
        snprintf(text, sizeof text, ": A - B is not positive definite (dpotrf stopped at the leading minor of order %d of %d): the %s "
                 "reference is unstable, and TDHF has no real excitation energies%s; the states are not returned", h, s.dim, s.ref, whom);
        return s.fail(TF_ELINALG, text);
    }
    return TF_OK;
}

// CIS: the eigenpairs of M in place (energies in d_w, state n = column n); the lowest nk vectors to x_out, zeros to y_out
static int cis_tda_solve(const CisSolve &s, double *M, const char *name, double *x_out, double *y_out)
{
    tf_ctx *ctx = s.ctx; const char *who = s.who;
    const int dim = s.dim, nk = s.nk;
    int h = 0;
    CIS_BLAS(rocsolver_dsyevd(s.blas, rocblas_evect_original, rocblas_fill_upper, dim, M, dim, s.d_w, s.d_e, s.d_info));
    if (!s.info(&h)) return s.fail(TF_ENODEVICE, ": the eigensolver failed on the device");
    if (h != 0) return s.fail(TF_ELINALG, std::string(": the eigenvalues of the ") + name + " CIS matrix did not converge (rocsolver_dsyevd)");
    if (nk > 0 && x_out && hipMemcpy(x_out, M, (size_t)nk * dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return s.fail(TF_ENODEVICE, ": copy failed");
    if (nk > 0 && y_out) std::fill(y_out, y_out + (size_t)nk * dim, 0.0);
    return TF_OK;
}

// TDHF with Mm = L of cis_tdhf_factor and M = A + B: M <- L^T (A + B) L, its eigenpairs (w^2, Z); energies in d_w; X + Y = L Z / sqrt(w)
// for every state in T (state n = column n), X and Y of the lowest nk to x_out, y_out.  Any w^2 <= 0: TF_ELINALG.
static int cis_tdhf_solve(const CisSolve &s, const double *Mm, double *M, const char *name, double *x_out, double *y_out)
{
    tf_ctx *ctx = s.ctx; const char *who = s.who;
    const int dim = s.dim, nk = s.nk;
    const long long B2 = (long long)dim * dim;
    const double one = 1.0;
    double *T = s.T, *Q = s.Q;
    int h = 0;
    CIS_BLAS(rocblas_dtrmm(s.blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, dim, dim, &one, Mm, dim, M,
                           dim, T, dim));
    CIS_BLAS(rocblas_dtrmm(s.blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit, dim, dim, &one, Mm, dim,
                           T, dim, M, dim));
    CIS_BLAS(rocsolver_dsyevd(s.blas, rocblas_evect_original, rocblas_fill_upper, dim, M, dim, s.d_w2, s.d_e, s.d_info));
    if (!s.info(&h)) return s.fail(TF_ENODEVICE, ": the eigensolver failed on the device");
    if (h != 0) return s.fail(TF_ELINALG, std::string(": the eigenvalues of the reduced ") + name + " TDHF matrix did not converge (rocsolver_dsyevd)");
    hipLaunchKernelGGL(tfcis::tdhf_roots_kernel, dim3(1), dim3(256), 0, 0, s.d_w2, dim, s.d_w, s.d_stat);
    double stat[2];
    if (hipMemcpy(stat, s.d_stat, sizeof stat, hipMemcpyDeviceToHost) != hipSuccess) return s.fail(TF_ENODEVICE, ": the root kernel failed on the device");
    if (stat[0] != 0.0) {
        char text[300];
        snprintf(text, sizeof text, ": %d %s root(s) of the TDHF problem have w^2 <= 0 (smallest w^2 = %.10g): the %s reference is "
                 "unstable towards a %s perturbation, and the states are not returned (CIS on the same orbitals still runs)", (int)stat[0], name, stat[1], s.ref,
                 name);
        return s.fail(TF_ELINALG, text);
    }
    // X + Y = L Z / sqrt(w) for every state; X - Y = sqrt(w) L^-T Z for the kept ones
    CIS_BLAS(rocblas_dtrmm(s.blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, dim, dim, &one, Mm, dim, M,
                           dim, T, dim));
    if (nk > 0) {
        if (hipMemcpy(Q, M, (size_t)nk * dim * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess) return s.fail(TF_ENODEVICE, ": copy failed");
        CIS_BLAS(rocblas_dtrsm(s.blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit, dim, nk, &one, Mm, dim,
                               Q, dim));
    }
    hipLaunchKernelGGL(tfcis::tdhf_backsub_kernel, dim3((unsigned)std::min<long long>((B2 + 255) / 256, 1 << 16)), dim3(256), 0, 0, T, Q, s.d_w, dim, nk, s.Xk,
                       s.Yk);
    if (nk > 0 && ((x_out && hipMemcpy(x_out, s.Xk, (size_t)nk * dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
                   (y_out && hipMemcpy(y_out, s.Yk, (size_t)nk * dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)))
        return s.fail(TF_ENODEVICE, ": copy failed");
    return TF_OK;
}

// The first out-of-memory message of a driver, its GB figure and its count of arrays from the plan; index = "(o v)" or "(d_alpha + d_beta)"
static int exc_work_oom(tf_ctx *ctx, const char *who, const ExcitedPlan &P, const char *index)
{
    char text[200];
    snprintf(text, sizeof text, "%s: out of device memory for %.2f GB of work space (%d arrays of %s^2 = %d^2 values)", who,
             (double)P.message * sizeof(double) / 1e9, P.n_square, index, P.dim);
    return corr_fail(ctx, TF_ENOMEM, text);
}

// The solve stages' view of a driver's plan and its small array and, unless P.tda, the dim^2 array of the triangular products
// and the kept vectors Q | Xk | Yk of the reduction (mem's)
static int cis_solve_begin(CisSolve &s, tf_ctx *ctx, const char *who, const char *ref, const ExcitedPlan &P, double *small, rocblas_int *d_info,
                           DeviceBlocks &mem)
{
    s.ctx = ctx; s.who = who; s.ref = ref; s.blas = ctx->scf.blas; s.dim = P.dim; s.nk = P.nk; s.d_info = d_info;
    s.d_w = P.at(small, EXC_W); s.d_w2 = P.at(small, EXC_W2); s.d_e = P.at(small, EXC_E); s.d_stat = P.at(small, EXC_STAT);
    if (P.tda) return TF_OK;
    s.T = mem.alloc(P.square);
    s.Q = s.T ? mem.alloc(3 * P.kept_rows) : nullptr;
    if (!s.Q) {
        char text[200];
        snprintf(text, sizeof text, "%s: out of device memory for %.2f GB of work space for the TDHF reduction", who, (double)(P.tdhf * sizeof(double)) / 1e9);
        return corr_fail(ctx, TF_ENOMEM, text);
    }
    s.Xk = s.Q + P.kept_rows; s.Yk = s.Xk + P.kept_rows;
    return TF_OK;
}

// D^c_ia = C_o^T D^c C_v for c = x, y, z of every spin with excitations (d[s] = o_s v_s > 0) into Dia[c][offset + i v + a] (rows of length
// dim, the spins side by side in the compound index): dip to the device once, then per spin C_o, C_v (the one pair of buffers serves the
// spins in turn) and two GEMMs per component through D C_v [N][v].  The restricted driver has one spin.
static int cis_dipoles(const CisSolve &sv, const ExcitedPlan &P, double *small, int N, const double *dip, int n_spins, const CorrSetup *S, const long long *d)
{
    tf_ctx *ctx = sv.ctx; const char *who = sv.who;
    double *d_Co = P.at(small, EXC_CO), *d_Cv = P.at(small, EXC_CV), *d_T1 = P.at(small, EXC_DCV), *d_Dia = P.at(small, EXC_DIA), *d_dip = P.at(small, EXC_DIP);
    if (hipMemcpy(d_dip, dip, 3 * (size_t)N * N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return sv.fail(TF_ENODEVICE, ": copy failed");
    size_t offset = 0;
    for (int s = 0; s < n_spins; ++s) {
        if (d[s] == 0) continue;
        if (hipMemcpy(d_Co, S[s].Co.data(), (size_t)N * S[s].o * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_Cv, S[s].Cv.data(), (size_t)N * S[s].v * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            return sv.fail(TF_ENODEVICE, ": copy failed");
        const int o = S[s].o, v = S[s].v;
        for (int c = 0; c < 3; ++c) {
            CIS_BLAS(tfmp3::gemm_rm(sv.blas, false, false, N, v, N, 1.0, d_dip + (size_t)c * N * N, N, d_Cv, v, 0.0, d_T1, v));
            CIS_BLAS(tfmp3::gemm_rm(sv.blas, true, false, o, v, N, 1.0, d_Co, o, d_T1, v, 0.0, d_Dia + (size_t)c * sv.dim + offset, v));
        }
        offset += (size_t)d[s];
    }
    return TF_OK;
}

// What TD-DFT adds to a driver, restricted or unrestricted: the fraction of exact exchange and the density P, or P_alpha and P_beta (host)
struct __attribute__((visibility("hidden"))) ExcXc { double hfx = 1.0; const double *P[2] = {nullptr, nullptr}; };

// ---- TD-DFT / TDA for the local-density functionals: the exchange-correlation kernel matrices (tf_xckernel.hip.h) ----------------------

static const char *const XCK_X_NAMES[4] = {"none", "Slater", "B88", "B3 (0.9 B88 + 0.1 Slater)"};
static const char *const XCK_C_NAMES[6] = {"none", "VWN5", "VWN3", "LYP", "3P (0.81 LYP + 0.19 VWN5)", "3P (0.81 LYP + 0.19 VWN3)"};

// What the kernel build needs besides the driver's own checks: a grid for this tensor, a local-density functional, the density of every
// spin, and a finite hfx (the entry points that build the kernel matrices alone pass 0: nothing of theirs is scaled by it)
static int xc_kernel_checks(tf_ctx *ctx, const char *who, const ExcXc &xc, int spins)
{
    const int rc = dft_grid_checks(ctx, who, " (the exchange-correlation kernel is integrated on its grid)", false);
    if (rc) return rc;
    const tfdft::Grid &g = ctx->grid;
    if (g.xid >= tfdft::X_B88 || g.cid >= tfdft::C_LYP)
        TF_FAIL(ctx, TF_EINVAL, "%s: the exchange-correlation kernel of exchange \"%s\" with correlation \"%s\" is not implemented: only the "
                "local-density functionals (Slater exchange, VWN3 / VWN5 correlation) have one", who, XCK_X_NAMES[g.xid], XCK_C_NAMES[g.cid]);
    if (!xc.P[0] || (spins == 2 && !xc.P[1])) TF_FAIL(ctx, TF_EINVAL, "%s: bad arguments (needs the density P)", who);
    if (ctx->world > 1) TF_FAIL(ctx, TF_EINVAL, "%s: a sharded tensor (world > 1) is not supported", who);
    if (!std::isfinite(xc.hfx)) TF_FAIL(ctx, TF_EINVAL, "%s: hfx must be finite", who);
    return TF_OK;
}

// The production path from psi to K: the plan, the slab partials (mem's, released here), xck_kernel and xck_sum_kernel on the null stream.
// psi [G][o + v] on the device.  seconds2: the K kernel, the slab sum (tf_xc_kernel_timings).
static int xc_kernel_matrices(tf_ctx *ctx, const char *who, long long G, int o, int v, const double *psi, const double *uS, const double *uT,
                              DeviceBlocks &mem, double *KS, double *KT, double *seconds2)
{
    const XckPlan P = xck_plan((long long)o * v, G);
    double *part = mem.alloc(P.partial_doubles);
    if (!part) {
        char text[200];
        snprintf(text, sizeof text, "%s: out of device memory for %.2f GB of slab partials (%d slabs of 2 x %lld^2 values)", who,
                 (double)P.partial_doubles * sizeof(double) / 1e9, P.n_slabs, P.dim);
        return corr_fail(ctx, TF_ENOMEM, text);
    }
    tfxck::Args A{psi, uS, uT, part, P.G, P.slab_len, o + v, o, v, (int)P.dim, P.n_b};
    const auto t0 = corr_stamp();
    hipLaunchKernelGGL(tfxck::xck_kernel, dim3((unsigned)P.n_tiles, (unsigned)P.n_slabs), dim3(XCK_THREADS), 0, 0, A);
    const auto t1 = corr_stamp();
    hipLaunchKernelGGL(tfxck::xck_sum_kernel, dim3((unsigned)((P.dim * P.dim + 255) / 256)), dim3(256), 0, 0, part, P.n_slabs, (int)P.dim, KS, KT);
    const auto t2 = corr_stamp();
    seconds2[0] = corr_secs(t1 - t0); seconds2[1] = corr_secs(t2 - t1);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": the exchange-correlation kernel build failed on the device");
    mem.release(part);
    return TF_OK;
}

// The orbital values of the windows of one CorrSetup on the grid: C_w = [C_o | C_v] [N][o + v] packed on the host and uploaded to Cw,
// psi [G][o + v] = Phi [G][N] C_w.  *t_psi gains the seconds of the GEMM; *t_end is the stamp after it.  The caller holds BlasAtomicsOff.
static int xc_orbital_windows(tf_ctx *ctx, const char *who, const CorrSetup &S, double *Cw, double *psi, double *t_psi, CorrTime *t_end)
{
    const int N = S.N, o = S.o, v = S.v, n = o + v;
    std::vector<double> hC((size_t)N * n);
    for (int m = 0; m < N; ++m) {
        std::copy(S.Co.begin() + (size_t)m * o, S.Co.begin() + (size_t)(m + 1) * o, hC.begin() + (size_t)m * n);
        std::copy(S.Cv.begin() + (size_t)m * v, S.Cv.begin() + (size_t)(m + 1) * v, hC.begin() + (size_t)m * n + o);
    }
    if (hipMemcpy(Cw, hC.data(), hC.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    const auto t0 = corr_stamp();
    CORR_BLAS(tfmp3::gemm_rm(ctx->scf.blas, false, false, (int)ctx->grid.G, n, N, 1.0, ctx->grid.b(tfdft::GB_PHI), N, Cw, n, 0.0, psi, n));
    *t_end = corr_stamp();
    *t_psi += corr_secs(*t_end - t0);
    return TF_OK;
}

// psi [n_o + n_v][G] as a probe passes it (psi_o, psi_v: one orbital after the other) to the production operand h [G][n_o + n_v]
static void xc_probe_repack(long long G, int n_o, int n_v, const double *psi_o, const double *psi_v, std::vector<double> &h)
{
    const int n = n_o + n_v;
    h.resize((size_t)G * n);
    for (long long g = 0; g < G; ++g) {
        for (int i = 0; i < n_o; ++i) h[(size_t)g * n + i] = psi_o[(size_t)i * G + g];
        for (int a = 0; a < n_v; ++a) h[(size_t)g * n + n_o + a] = psi_v[(size_t)a * G + g];
    }
}

// K_S, K_T [dim][dim] (mem's) for the windows of S, the density P (host) and the grid's functional; f_points (host, may be null):
// [4][G] = rho, f_X, f_C^S, f_C^T.  ctx->xck_seconds: psi GEMM, density + point kernels, K kernel, slab sum.
static int xc_kernel_build(tf_ctx *ctx, const char *who, const CorrSetup &S, const double *P, DeviceBlocks &mem, double **pKS, double **pKT,
                           double *f_points)
{
    double *seconds4 = ctx->xck_seconds;
    tfdft::Grid &g = ctx->grid;
    const int N = S.N, o = S.o, v = S.v, n = o + v;
    const long long G = g.G;
    const size_t dd = (size_t)S.B2;
    rocblas_handle blas = ctx->scf.blas;
    double *KS = mem.alloc(dd), *KT = mem.alloc(dd), *u = mem.alloc(2 * (size_t)G), *psi = mem.alloc((size_t)G * n), *Cw = mem.alloc((size_t)N * n),
           *fp = f_points ? mem.alloc(4 * (size_t)G) : nullptr;
    if (!KS || !KT || !u || !psi || !Cw || (f_points && !fp)) {
        char text[200];
        snprintf(text, sizeof text, "%s: out of device memory for %.2f GB of work space of the exchange-correlation kernel (2 x %lld^2 values and "
                 "%lld x %d orbital values)", who, (double)(2 * dd + (size_t)G * (n + 6) + (size_t)N * n) * sizeof(double) / 1e9, S.ov, G, n);
        return corr_fail(ctx, TF_ENOMEM, text);
    }
    if (hipMemcpy(ctx->jk.all.P, P, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    BlasAtomicsOff no_atomics(blas);
    CorrTime t1;
    double t_psi = 0.0;
    int rc = xc_orbital_windows(ctx, who, S, Cw, psi, &t_psi, &t1);
    if (rc) return rc;
    // rho through the density stage of V_XC (its GEMM is the rocblas_dgemm call tfmp3::gemm_rm made here); then the point kernels
    CORR_BLAS(tfdft::density_stage(blas, g, ctx->jk.all.P, 0));
    hipLaunchKernelGGL(tfdft::xc_fpoint_kernel, dim3((unsigned)((G + 127) / 128)), dim3(128), 0, 0, G, g.xid, g.cid, g.dfx, g.dfc, g.x_alpha,
                       g.b(tfdft::GB_RHO), g.b(tfdft::GB_W), u, u + G, fp);
    const auto t2 = corr_stamp();
    seconds4[0] = t_psi; seconds4[1] = corr_secs(t2 - t1);
    if ((rc = xc_kernel_matrices(ctx, who, G, o, v, psi, u, u + G, mem, KS, KT, seconds4 + 2))) return rc;
    if (f_points && hipMemcpy(f_points, fp, 4 * (size_t)G * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    mem.release(u); mem.release(psi); mem.release(Cw); mem.release(fp);
    *pKS = KS; *pKT = KT;
    return TF_OK;
}

int tf_xc_kernel_plan(int64_t dim, int64_t n_points, int64_t out[8])
{
    if (dim < 1 || n_points < 1 || !out) return TF_EINVAL;
    const XckPlan P = xck_plan(dim, n_points);
    out[0] = P.n_b; out[1] = P.n_tiles; out[2] = P.n_slabs; out[3] = P.slab_len; out[4] = (int64_t)P.lds_bytes; out[5] = XCK_CHUNK;
    out[6] = XCK_SLAB_MIN; out[7] = XCK_TILE;
    return TF_OK;
}

int tf_xc_kernel_timings(tf_ctx *ctx, double out[4])
{
    if (!ctx || !out) return TF_EINVAL;
    std::copy(ctx->xck_seconds, ctx->xck_seconds + 4, out);
    return TF_OK;
}

int tf_xc_kernel_probe(tf_ctx *ctx, int n_o, int n_v, int64_t n_points, const double *psi_o, const double *psi_v, const double *u_singlet,
                       const double *u_triplet, double *K_singlet, double *K_triplet)
{
    static const char *who = "tf_xc_kernel_probe";
    if (!ctx) return TF_EINVAL;
    if (n_o < 1 || n_v < 1 || n_points < 1 || !psi_o || !psi_v || !u_singlet || !u_triplet || !K_singlet || !K_triplet)
        TF_FAIL(ctx, TF_EINVAL, "%s: bad arguments (needs n_o, n_v, n_points >= 1 and every pointer)", who);
    const long long ov = (long long)n_o * n_v, G = n_points;
    if (ov > 2000000LL || (long long)G * (n_o + n_v) > (1LL << 40)) TF_FAIL(ctx, TF_EINVAL, "%s: dimension overflow", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int n = n_o + n_v;
    const size_t dd = (size_t)ov * ov;
    DeviceBlocks mem;
    double *psi = mem.alloc((size_t)G * n), *u = mem.alloc(2 * (size_t)G), *KS = mem.alloc(dd), *KT = mem.alloc(dd);
    if (!psi || !u || !KS || !KT) TF_FAIL(ctx, TF_ENOMEM, "%s: out of device memory for %.2f GB", who, (double)((size_t)G * (n + 2) + 2 * dd) * 8 / 1e9);
    std::vector<double> h;                                    // the production operand: psi [G][o + v]
    xc_probe_repack(G, n_o, n_v, psi_o, psi_v, h);
    if (hipMemcpy(psi, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(u, u_singlet, (size_t)G * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(u + G, u_triplet, (size_t)G * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    ctx->xck_seconds[0] = ctx->xck_seconds[1] = 0.0;
    const int rc = xc_kernel_matrices(ctx, who, G, n_o, n_v, psi, u, u + G, mem, KS, KT, ctx->xck_seconds + 2);
    if (rc) return rc;
    if (hipMemcpy(K_singlet, KS, dd * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(K_triplet, KT, dd * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    return TF_OK;
}

int tf_xc_kernel_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *P, double *K_singlet, double *K_triplet, double *f_points)
{
    static const char *who = "tf_xc_kernel_rhf";
    int rc = corr_args(ctx, who, C && K_singlet && K_triplet, " (needs C, K_singlet, K_triplet and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    const ExcXc xc{0.0, {P, nullptr}};
    if ((rc = xc_kernel_checks(ctx, who, xc, 1))) return rc;
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    if (S.ov > 2000000LL) TF_FAIL(ctx, TF_EINVAL, "%s: dimension overflow", who);
    DeviceBlocks mem;
    double *KS = nullptr, *KT = nullptr;
    if ((rc = xc_kernel_build(ctx, who, S, P, mem, &KS, &KT, f_points))) return rc;
    if (hipMemcpy(K_singlet, KS, (size_t)S.B2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(K_triplet, KT, (size_t)S.B2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    return TF_OK;
}

// The restricted matrix stage, the counterpart of ucis_mo_blocks + ucis_assemble.  One matrix of the assembly pass: its kind in
// tfcis::assemble, the kernel matrix it gains kfac times (may be null) and where it goes (null: not asked for)
struct CisMatrix { int kind; const double *K; double kfac; double *out; };

struct __attribute__((visibility("hidden"))) CisBlocks {
    double *g1 = nullptr, *g2 = nullptr, *Ht = nullptr, *KS = nullptr, *KT = nullptr, hfx = 1.0;
    CorrTime t1;                 // after the MO blocks
};

// The MO blocks as tf_mp3_rhf makes them ((ki|lj) is not needed here), without exact exchange (ia|jb) alone; then -- TD-DFT, unless the
// grid's functional is the null one -- K_S / K_T of xc_kernel_build; then the array of the transposed (ij|ab), which the driver tests
// together with its own allocations, so that one message reports them all
static int cis_mo_blocks(tf_ctx *ctx, const char *who, const CorrSetup &S, const ExcXc *xc, DeviceBlocks &mem, CisBlocks &B)
{
    int rc;
    B.hfx = xc ? xc->hfx : 1.0;
    if (B.hfx == 0.0) {
        if ((rc = mo_transform_device(ctx, S.Co.data(), S.o, S.Cv.data(), S.v, S.Co.data(), S.o, S.Cv.data(), S.v, mem, &B.g1, nullptr))) return rc;
    } else {
        double *g3 = nullptr;
        if ((rc = mp3_mo_blocks(ctx, who, S, mem, &B.g1, &B.g2, &g3))) return rc;
        mem.release(g3);
    }
    B.t1 = corr_stamp();
    if (xc && (ctx->grid.xid != 0 || ctx->grid.cid != 0) && (rc = xc_kernel_build(ctx, who, S, xc->P[0], mem, &B.KS, &B.KT, nullptr))) return rc;
    B.Ht = B.g2 ? mem.alloc((size_t)S.B2) : nullptr;
    return TF_OK;
}

// eps to d_eps [N], (ab|ij) transposed to [(ij)][(ab)] and the n matrices of M assembled in one pass, after which the blocks, Ht and the
// kernel matrices are freed
static int cis_assemble(tf_ctx *ctx, const char *who, const CorrSetup &S, DeviceBlocks &mem, const CisBlocks &B, const double *eps, double *d_eps,
                        const CisMatrix *M, int n)
{
    if (hipMemcpy(d_eps, eps, (size_t)S.N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    if (B.g2) tfcis::launch_transpose(B.g2, (long long)S.v * S.v, (long long)S.o * S.o, B.Ht, 0);
    tfcis::AssembleArgs A{};
    A.g1 = B.g1; A.Ht = B.Ht; A.eps = d_eps; A.n_frozen = S.n_frozen; A.n_occ = S.n_occ; A.o = S.o; A.v = S.v;
    A.hfx = B.hfx;
    for (int m = 0; m < n; ++m)
        if (M[m].out) { A.kind[A.n_out] = M[m].kind; A.K[A.n_out] = M[m].K; A.kfac[A.n_out] = M[m].kfac; A.out[A.n_out++] = M[m].out; }
    tfcis::launch_assemble(A, 0);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": the assembly kernels failed on the device");
    mem.release(B.g1); mem.release(B.g2); mem.release(B.Ht); mem.release(B.KS); mem.release(B.KT);
    return TF_OK;
}

// Closed-shell CIS / TDHF (tuna_ci.py:719-841, :1161-1211, :1284-1366, :1466-1518; tf_cis.hip.h has the matrices and the reduction).
// Stages: the MO blocks of tf_mp3_rhf; (ab|ij) transposed to [(ij)][(ab)] and every matrix of the call assembled in one pass, after which
// the blocks are freed; then per multiplicity one dsyevd (CIS), or dpotrf of A - B once and per multiplicity two dtrmm, one dsyevd, one
// dtrmm and -- for the kept states -- one dtrsm (TDHF); the transition moments of the singlets as GEMMs.  All dim x dim arrays of the
// solves are symmetric or read column by column (state n = column n = dim contiguous values), so rocSOLVER's column-major view needs no
// transposition.
// tf_tddft_rhf is the same driver with xc set: the exchange blocks scaled by hfx ((ab|ij) not built when hfx = 0) and, unless the grid's
// functional is the null one, K_S / K_T of xc_kernel_build added in the assembly pass (counted in the assembly slot of seconds).
static int cis_rhf_driver(tf_ctx *ctx, const char *who, const tf_cis_opts *opts, const ExcXc *xc, int n_occ, int n_frozen, const double *C,
                          const double *eps, const double *dip, tf_cis_result *out)
{
    const std::string me = who;
    int rc = corr_args(ctx, who, opts && C && eps && out, " (needs opts, C, eps, out and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    if (!opts->singlets && !opts->triplets) TF_FAIL(ctx, TF_EINVAL, "%s: neither singlets nor triplets asked for: there are no excited states to calculate", who);
    if (opts->n_keep < 0) TF_FAIL(ctx, TF_EINVAL, "%s: n_keep must not be negative", who);
    if ((out->tdm || out->osc) && !dip) TF_FAIL(ctx, TF_EINVAL, "%s: transition dipoles and oscillator strengths need the AO dipole matrices (dip)", who);
    if (xc && (rc = xc_kernel_checks(ctx, who, *xc, 1))) return rc;
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const long long B2 = S.B2;
    if (S.ov > 2000000LL || (long long)S.v * S.v > 2000000LL) TF_FAIL(ctx, TF_EINVAL, "%s: dimension overflow", who);   // (grids of 32-wide tiles)
    const int N = S.N, dim = (int)S.ov, nk = std::min(opts->n_keep, dim);
    const bool tda = opts->tda != 0, sing = opts->singlets != 0, trip = opts->triplets != 0, moments = sing && dip && (out->tdm || out->osc);
    out->dim = dim;
    DeviceBlocks mem;
    // ---- MO blocks and the exchange-correlation kernel matrices (TD-DFT)
    CisBlocks B;
    if ((rc = cis_mo_blocks(ctx, who, S, xc, mem, B))) return rc;
    // ---- work space: the matrices (CIS: A per multiplicity; TDHF: A + B per multiplicity, A - B and one more dim^2 array for the
    //      triangular products), the transposed (ij|ab) until the assembly is done, the kept vectors, and the small arrays of the plan
    const ExcitedPlan P = excited_plan_rhf(N, S.o, S.v, tda, sing, trip, nk);
    double *Ms = sing ? mem.alloc((size_t)B2) : nullptr, *Mt = trip ? mem.alloc((size_t)B2) : nullptr, *Mm = tda ? nullptr : mem.alloc((size_t)B2),
           *small = mem.alloc(P.total);
    rocblas_int *d_info = mem.alloc_int(4);
    if ((B.g2 && !B.Ht) || (sing && !Ms) || (trip && !Mt) || (!tda && !Mm) || !small || !d_info) return exc_work_oom(ctx, who, P, "(o v)");
    // ---- assembly
    const double kf = tda ? 1.0 : 2.0;                            // A gains K, A + B gains 2 K, A - B nothing
    const CisMatrix Ma[3] = {{tda ? 0 : 2, B.KS, kf, Ms}, {tda ? 1 : 3, B.KT, kf, Mt}, {4, nullptr, 0.0, Mm}};
    if ((rc = cis_assemble(ctx, who, S, mem, B, eps, P.at(small, EXC_EPS), Ma, 3))) return rc;
    const std::pair<double *, const double *> outs[3] = {{out->m_plus_singlet, Ms}, {out->m_plus_triplet, Mt}, {out->m_minus, Mm}};
    for (const auto &pr : outs)
        if (pr.first && pr.second && hipMemcpy(pr.first, pr.second, (size_t)B2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            return corr_fail(ctx, TF_ENODEVICE, me + ": copy failed");
    const auto t2 = corr_stamp();
    // ---- solves (the stages shared with tf_cis_uhf)
    CisSolve sv;
    if ((rc = cis_solve_begin(sv, ctx, who, "RHF", P, small, d_info, mem))) return rc;
    BlasAtomicsOff no_atomics(sv.blas);                       // no atomics in the products: split-K sums would change from run to run
    if (moments && (rc = cis_dipoles(sv, P, small, N, dip, 1, &S, &S.ov))) return rc;              // D^c_ia = C_o^T D^c C_v
    if (!tda && (rc = cis_tdhf_factor(sv, Mm, " for singlets or triplets"))) return rc;             // A - B = L L^T, once for both multiplicities
    for (int mult = 0; mult < 2; ++mult) {
        double *M = mult == 0 ? Ms : Mt;
        if (!M) continue;
        const char *name = mult == 0 ? "singlet" : "triplet";
        double *e_out = mult == 0 ? out->e_singlet : out->e_triplet, *x_out = mult == 0 ? out->x_singlet : out->x_triplet,
               *y_out = mult == 0 ? out->y_singlet : out->y_triplet;
        if ((rc = tda ? cis_tda_solve(sv, M, name, x_out, y_out) : cis_tdhf_solve(sv, Mm, M, name, x_out, y_out))) return rc;
        const double *V = tda ? M : sv.T;                         // the transition vectors X + Y, state by state
        if (e_out && hipMemcpy(e_out, sv.d_w, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, me + ": copy failed");
        // mu_n[c] = sqrt(2) sum_ia D^c_ia V[ia][n]
        if (mult == 0 && moments && (rc = cis_transition_moments(sv, P, small, V, std::sqrt(2.0), out->tdm, out->osc))) return rc;
    }
    if (hipGetLastError() != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, me + ": a kernel launch failed");
    corr_stage_seconds(out->seconds, S.t0, B.t1, t2, corr_stamp());
    return TF_OK;
}

int tf_cis_rhf(tf_ctx *ctx, const tf_cis_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, const double *dip, tf_cis_result *out)
{
    return cis_rhf_driver(ctx, "tf_cis_rhf", opts, nullptr, n_occ, n_frozen, C, eps, dip, out);
}

int tf_tddft_rhf(tf_ctx *ctx, const tf_tddft_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, const double *P,
                 const double *dip, tf_cis_result *out)
{
    tf_cis_opts co{};
    ExcXc xc;
    if (opts) { co.tda = opts->tda; co.singlets = opts->singlets; co.triplets = opts->triplets; co.n_keep = opts->n_keep; xc.hfx = opts->hfx; }
    xc.P[0] = P;
    return cis_rhf_driver(ctx, "tf_tddft_rhf", opts ? &co : nullptr, &xc, n_occ, n_frozen, C, eps, dip, out);
}

// ---- unrestricted CIS / TDHF and the stability analysis ----------------------------------------------------------------------------

// The prologue of a driver on UHF orbitals: the checks, one rank only, the device, the start of the clock, the SCF work space and the
// windows of either spin.  An empty spin block (o_s = 0 or v_s = 0) is allowed; dim = 0 is not.
struct __attribute__((visibility("hidden"))) UcisSetup {
    CorrSetup s[2];                                           // alpha, beta
    int N = 0, dim = 0;
    long long d[2] = {0, 0};                                  // o_s v_s
    CorrTime t0;
};

static int ucis_begin(tf_ctx *ctx, const char *who, bool pointers_ok, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha,
                      const double *C_beta, UcisSetup &U)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "%s: call tf_build_eri first", who);
    const int N = ctx->N;
    if (!pointers_ok || n_frozen_alpha < 0 || n_frozen_alpha > n_alpha || n_alpha > N || n_frozen_beta < 0 || n_frozen_beta > n_beta || n_beta > N)
        TF_FAIL(ctx, TF_EINVAL, "%s: bad arguments (needs every pointer but dip, and 0 <= n_frozen <= n <= N for both spins)", who);
    const long long da = (long long)(n_alpha - n_frozen_alpha) * (N - n_alpha), db = (long long)(n_beta - n_frozen_beta) * (N - n_beta);
    if (da + db == 0) TF_FAIL(ctx, TF_EINVAL, "%s: no spin-conserving excitation (o v = 0 for both spins): there is nothing to calculate", who);
    if (da + db > 2000000LL) TF_FAIL(ctx, TF_EINVAL, "%s: dimension overflow", who);                      // (grids of 32-wide tiles)
    if (ctx->world > 1) TF_FAIL(ctx, TF_EINVAL, "%s: a sharded tensor (world > 1) is not supported", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    U.t0 = std::chrono::steady_clock::now();
    std::string msg;
    const int rc = tfscf::ensure(ctx->scf, N, 6, msg);
    if (rc) { ctx->err = msg; return rc; }
    U.N = N; U.d[0] = da; U.d[1] = db; U.dim = (int)(da + db);
    U.s[0].windows(N, n_alpha, n_frozen_alpha, C_alpha);
    U.s[1].windows(N, n_beta, n_frozen_beta, C_beta);
    return TF_OK;
}

// The five MO blocks of tfucis::uassemble_kernel through the general transformation, on every layout (mem's): per spin with d_s > 0
// (ia|jb) and -- with_H -- (ab|ij), the latter transposed to [i][j][a][b]; (ia alpha|jb beta) when both spins have excitations.  Without
// exact exchange (with_H false) the two (ab|ij) blocks are neither built nor read.
static int ucis_mo_blocks(tf_ctx *ctx, const char *who, const UcisSetup &U, DeviceBlocks &mem, tfucis::AssembleArgs &A, bool with_H = true)
{
    int rc;
    for (int s = 0; s < 2; ++s) {
        if (U.d[s] == 0) continue;
        const CorrSetup &S = U.s[s];
        const int o = S.o, v = S.v;
        double *g = nullptr;
        if ((rc = mo_transform_device(ctx, S.Co.data(), o, S.Cv.data(), v, S.Co.data(), o, S.Cv.data(), v, mem, &g, nullptr))) return rc;
        A.s[s].g = g;
        if (!with_H) continue;
        double *g2 = mem.alloc((size_t)v * v * o * o), *Ht = g2 ? mem.alloc((size_t)v * v * o * o) : nullptr;
        if (!Ht) {
            char text[200];
            snprintf(text, sizeof text, "%s: out of device memory for %.2f GB of work space ((ab|ij) of one spin in two orders)", who,
                     2.0 * (double)v * v * o * o * sizeof(double) / 1e9);
            return corr_fail(ctx, TF_ENOMEM, text);
        }
        if ((rc = mo_vvoo_block(ctx, who, S.Cv, S.Cv, S.Co, S.Co, o, v, g2))) return rc;
        tfcis::launch_transpose(g2, (long long)v * v, (long long)o * o, Ht, 0);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": the transposition of (ab|ij) failed on the device");
        mem.release(g2);
        A.s[s].Ht = Ht;
    }
    if (U.d[0] > 0 && U.d[1] > 0) {
        double *g = nullptr;
        if ((rc = mo_transform_device(ctx, U.s[0].Co.data(), U.s[0].o, U.s[0].Cv.data(), U.s[0].v, U.s[1].Co.data(), U.s[1].o, U.s[1].Cv.data(), U.s[1].v, mem,
                                      &g, nullptr)))
            return rc;
        A.g_ab = g;
    }
    return TF_OK;
}

// One assembly pass: the matrices A.out of kinds A.kind from the blocks of ucis_mo_blocks, which are freed afterwards; d_eps = 2 N doubles
static int ucis_assemble(tf_ctx *ctx, const char *who, const UcisSetup &U, DeviceBlocks &mem, tfucis::AssembleArgs &A, const double *eps_alpha,
                         const double *eps_beta, double *d_eps)
{
    const int N = U.N;
    if (hipMemcpy(d_eps, eps_alpha, (size_t)N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_eps + N, eps_beta, (size_t)N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    for (int s = 0; s < 2; ++s) {
        A.s[s].eps = d_eps + (size_t)s * N;
        A.s[s].n_frozen = U.s[s].n_frozen; A.s[s].n_occ = U.s[s].n_occ;
        A.s[s].o = U.d[s] ? U.s[s].o : 0; A.s[s].v = U.d[s] ? U.s[s].v : 0;     // an empty block: d_s = 0 in the kernel whichever of o, v is 0
    }
    tfucis::launch_uassemble(A, 0);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": the assembly kernel failed on the device");
    for (int s = 0; s < 2; ++s) { mem.release((void *)A.s[s].g); mem.release((void *)A.s[s].Ht); }
    mem.release((void *)A.g_ab);
    return TF_OK;
}

// ---- unrestricted TD-DFT / TDA and the Kohn-Sham stability analysis: the spin-blocked kernel matrix (tf_xckernel.hip.h) ------------------

// The production path from psi of both spins to K: the plan, the slab partials (mem's, released here), xck_spin_kernel and
// xck_spin_sum_kernel on the null stream.  psi[s] [G][o_s + v_s] on the device (not read when d_s = 0), u [3][G] = u_aa, u_ab, u_bb.
// seconds2: the K kernel, the slab sum (tf_xc_kernel_timings).
static int xc_kernel_spin_matrices(tf_ctx *ctx, const char *who, long long G, const int o[2], const int v[2], const double *const psi[2], const double *u,
                                   DeviceBlocks &mem, double *K, double *seconds2)
{
    const XckSpinPlan P = xck_spin_plan((long long)o[0] * v[0], (long long)o[1] * v[1], G, ctx->xck_spin_cols ? ctx->xck_spin_cols : XCK_SPIN_COLS);
    if (P.lds_bytes > XCK_LDS_LIMIT) return corr_fail(ctx, TF_EINVAL, std::string(who) + ": the kernel build's LDS carve-out exceeds the workgroup's");
    double *part = mem.alloc(P.partial_doubles);
    rocblas_int *d_tiles = mem.alloc_int(3 * (size_t)P.n_tiles);
    if (!part || !d_tiles) {
        char text[200];
        snprintf(text, sizeof text, "%s: out of device memory for %.2f GB of slab partials (%d slabs of %lld^2 values)", who,
                 (double)P.partial_doubles * sizeof(double) / 1e9, P.n_slabs, P.dim);
        return corr_fail(ctx, TF_ENOMEM, text);
    }
    tfxck::SpinArgs A{};
    for (int s = 0; s < 2; ++s) {
        A.psi[s] = P.d[s] ? psi[s] : nullptr;
        A.n[s] = o[s] + v[s]; A.o[s] = o[s]; A.v[s] = v[s]; A.d[s] = (int)P.d[s]; A.n_b[s] = P.n_b[s];
    }
    A.u[0] = u; A.u[1] = u + G; A.u[2] = u + 2 * G;
    A.part = part; A.G = P.G; A.slab_len = P.slab_len; A.dim = (int)P.dim;
    {
        std::vector<XckSpinTile> tiles((size_t)P.n_tiles);    // the plan's list: {row block, first column block, column blocks} per tile
        xck_spin_tiles(P, tiles.data());
        static_assert(sizeof(XckSpinTile) == 3 * sizeof(rocblas_int), "XckSpinTile is three ints");
        if (hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(XckSpinTile), hipMemcpyHostToDevice) != hipSuccess)
            return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
        A.tiles = d_tiles;
    }
    const auto t0 = corr_stamp();
    if (P.cols == 2) hipLaunchKernelGGL(tfxck::xck_spin_kernel<2>, dim3((unsigned)P.n_tiles, (unsigned)P.n_slabs), dim3(XCK_THREADS), 0, 0, A);
    else hipLaunchKernelGGL(tfxck::xck_spin_kernel<1>, dim3((unsigned)P.n_tiles, (unsigned)P.n_slabs), dim3(XCK_THREADS), 0, 0, A);
    const auto t1 = corr_stamp();
    hipLaunchKernelGGL(tfxck::xck_spin_sum_kernel, dim3((unsigned)((P.dim * P.dim + 255) / 256)), dim3(256), 0, 0, part, P.n_slabs, (int)P.dim, K);
    const auto t2 = corr_stamp();
    seconds2[0] = corr_secs(t1 - t0); seconds2[1] = corr_secs(t2 - t1);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": the exchange-correlation kernel build failed on the device");
    mem.release(part); mem.release(d_tiles);
    return TF_OK;
}

// K [dim][dim] (mem's) for the windows of U, the spin densities Pa, Pb (host) and the grid's functional; f_points (host, may be null):
// [7][G] = rho_a, rho_b, f_X,aa, f_X,bb, f_C,aa, f_C,ab, f_C,bb.  ctx->xck_seconds: psi GEMMs, densities + point kernels, K kernel, slab sum.
static int xc_kernel_spin_build(tf_ctx *ctx, const char *who, const UcisSetup &U, const double *Pa, const double *Pb, DeviceBlocks &mem, double **pK,
                                double *f_points)
{
    double *seconds4 = ctx->xck_seconds;
    tfdft::Grid &g = ctx->grid;
    const int N = U.N;
    const long long G = g.G;
    const size_t dd = (size_t)U.dim * U.dim, nn = (size_t)N * N;
    rocblas_handle blas = ctx->scf.blas;
    std::string msg;
    int rc = tfdft::ensure_spin(g, msg);
    if (rc) { ctx->err = std::string(who) + ": " + msg; return rc; }
    int o[2], v[2], n[2];
    for (int s = 0; s < 2; ++s) { o[s] = U.d[s] ? U.s[s].o : 0; v[s] = U.d[s] ? U.s[s].v : 0; n[s] = o[s] + v[s]; }
    const int nmax = std::max(n[0], n[1]);
    double *K = mem.alloc(dd), *u = mem.alloc(3 * (size_t)G), *psi[2] = {n[0] ? mem.alloc((size_t)G * n[0]) : nullptr, n[1] ? mem.alloc((size_t)G * n[1]) : nullptr},
           *Cw = mem.alloc((size_t)N * nmax), *fp = f_points ? mem.alloc(7 * (size_t)G) : nullptr;
    if (!K || !u || (n[0] && !psi[0]) || (n[1] && !psi[1]) || !Cw || (f_points && !fp)) {
        char text[240];
        snprintf(text, sizeof text, "%s: out of device memory for %.2f GB of work space of the exchange-correlation kernel (%d^2 values and "
                 "%lld x %d orbital values)", who, (double)(dd + (size_t)G * (n[0] + n[1] + 10) + (size_t)N * nmax) * sizeof(double) / 1e9, U.dim, G, n[0] + n[1]);
        return corr_fail(ctx, TF_ENOMEM, text);
    }
    double *io = g.s(tfdft::GS_IO);
    if (hipMemcpy(io, Pa, nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(io + nn, Pb, nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    BlasAtomicsOff no_atomics(blas);
    double t_psi = 0.0;
    // psi_s [G][n_s] = Phi [G][N] [C_o | C_v] of spin s [N][n_s]
    for (int s = 0; s < 2; ++s) {
        if (!n[s]) continue;
        CorrTime t_end;
        if ((rc = xc_orbital_windows(ctx, who, U.s[s], Cw, psi[s], &t_psi, &t_end))) return rc;
    }
    const auto t1 = corr_stamp();
    // rho_a, rho_b through the spin density stage of the unrestricted V_XC; then the point kernels
    CORR_BLAS(tfdft::density2_stage(blas, g, io, io + nn, 0));
    hipLaunchKernelGGL(tfdft::xc_fpoint2_kernel, dim3((unsigned)((G + 127) / 128)), dim3(128), 0, 0, G, g.xid, g.cid, g.dfx, g.dfc, g.x_alpha,
                       g.s(tfdft::GS_PT), g.b(tfdft::GB_W), u, fp);
    const auto t2 = corr_stamp();
    seconds4[0] = t_psi; seconds4[1] = corr_secs(t2 - t1);
    rc = xc_kernel_spin_matrices(ctx, who, G, o, v, psi, u, mem, K, seconds4 + 2);
    if (rc) return rc;
    if (f_points && hipMemcpy(f_points, fp, 7 * (size_t)G * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    mem.release(u); mem.release(psi[0]); mem.release(psi[1]); mem.release(Cw); mem.release(fp);
    *pK = K;
    return TF_OK;
}

int tf_xc_kernel_spin_plan(int64_t d_alpha, int64_t d_beta, int64_t n_points, int64_t out[8])
{
    if (d_alpha < 0 || d_beta < 0 || d_alpha + d_beta < 1 || n_points < 1 || !out) return TF_EINVAL;
    const XckSpinPlan P = xck_spin_plan(d_alpha, d_beta, n_points);
    out[0] = P.n_b[0]; out[1] = P.n_b[1]; out[2] = P.n_tiles; out[3] = P.n_slabs; out[4] = P.slab_len; out[5] = (int64_t)P.lds_bytes;
    out[6] = (int64_t)P.partial_doubles; out[7] = XCK_TILE * P.cols;
    return TF_OK;
}

int tf_xc_kernel_spin_cols(tf_ctx *ctx, int cols)
{
    if (!ctx) return TF_EINVAL;
    if (cols < 0 || cols > 2) TF_FAIL(ctx, TF_EINVAL, "tf_xc_kernel_spin_cols: cols must be 0 (the default shape), 1 (64 x 64 tiles) or 2 (64 x 128 tiles)");
    ctx->xck_spin_cols = cols;
    return TF_OK;
}

int tf_xc_kernel_spin_probe(tf_ctx *ctx, int o_a, int v_a, int o_b, int v_b, int64_t n_points, const double *psi_oa, const double *psi_va,
                            const double *psi_ob, const double *psi_vb, const double *u_aa, const double *u_ab, const double *u_bb, double *K)
{
    static const char *who = "tf_xc_kernel_spin_probe";
    if (!ctx) return TF_EINVAL;
    if (o_a < 0 || v_a < 0 || o_b < 0 || v_b < 0 || n_points < 1 || !u_aa || !u_ab || !u_bb || !K)
        TF_FAIL(ctx, TF_EINVAL, "%s: bad arguments (needs sizes >= 0, n_points >= 1 and u_aa, u_ab, u_bb, K)", who);
    const long long da = (long long)o_a * v_a, db = (long long)o_b * v_b, G = n_points;
    if (da + db == 0) TF_FAIL(ctx, TF_EINVAL, "%s: no element (o v = 0 for both spins): there is nothing to calculate", who);
    if ((da && (!psi_oa || !psi_va)) || (db && (!psi_ob || !psi_vb))) TF_FAIL(ctx, TF_EINVAL, "%s: bad arguments (a spin with o v > 0 needs its psi_o and psi_v)", who);
    if (da + db > 2000000LL || (long long)G * ((long long)o_a + v_a + o_b + v_b) > (1LL << 40)) TF_FAIL(ctx, TF_EINVAL, "%s: dimension overflow", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int o[2] = {da ? o_a : 0, db ? o_b : 0}, v[2] = {da ? v_a : 0, db ? v_b : 0};
    const double *po[2] = {psi_oa, psi_ob}, *pv[2] = {psi_va, psi_vb};
    const size_t dd = (size_t)(da + db) * (size_t)(da + db);
    DeviceBlocks mem;
    double *psi[2] = {nullptr, nullptr}, *u = mem.alloc(3 * (size_t)G), *Kd = mem.alloc(dd);
    bool ok = u && Kd;
    for (int s = 0; s < 2 && ok; ++s)
        if (o[s]) { psi[s] = mem.alloc((size_t)G * (o[s] + v[s])); ok = psi[s] != nullptr; }
    if (!ok) TF_FAIL(ctx, TF_ENOMEM, "%s: out of device memory for %.2f GB", who, (double)((size_t)G * (o[0] + v[0] + o[1] + v[1] + 3) + dd) * 8 / 1e9);
    for (int s = 0; s < 2; ++s) {
        if (!o[s]) continue;
        std::vector<double> h;                                // the production operand: psi [G][o + v]
        xc_probe_repack(G, o[s], v[s], po[s], pv[s], h);
        if (hipMemcpy(psi[s], h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    }
    if (hipMemcpy(u, u_aa, (size_t)G * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(u + G, u_ab, (size_t)G * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(u + 2 * G, u_bb, (size_t)G * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    ctx->xck_seconds[0] = ctx->xck_seconds[1] = 0.0;
    const int rc = xc_kernel_spin_matrices(ctx, who, G, o, v, psi, u, mem, Kd, ctx->xck_seconds + 2);
    if (rc) return rc;
    if (hipMemcpy(K, Kd, dd * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    return TF_OK;
}

int tf_xc_kernel_uhf(tf_ctx *ctx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha, const double *C_beta,
                     const double *P_alpha, const double *P_beta, double *K, double *f_points)
{
    static const char *who = "tf_xc_kernel_uhf";
    UcisSetup U;
    int rc = ucis_begin(ctx, who, C_alpha && C_beta && K, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, C_alpha, C_beta, U);
    if (rc) return rc;
    const ExcXc xc{0.0, {P_alpha, P_beta}};
    if ((rc = xc_kernel_checks(ctx, who, xc, 2))) return rc;
    DeviceBlocks mem;
    double *Kd = nullptr;
    if ((rc = xc_kernel_spin_build(ctx, who, U, P_alpha, P_beta, mem, &Kd, f_points))) return rc;
    if (hipMemcpy(K, Kd, (size_t)U.dim * U.dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    return TF_OK;
}

// Unrestricted CIS / TDHF (tuna_ci.py:755-757, :823-825, :1377-1455, :1529-1571; tf_ucis.hip.h has the matrices).  Stages: the five MO
// blocks; every matrix of the call assembled in one pass, after which the blocks are freed; then the solve stages of tf_cis_rhf on the
// spin-blocked matrices (CIS: one dsyevd; TDHF: dpotrf of A - B, two dtrmm, dsyevd, dtrmm, and dtrsm for the kept states); the
// transition moments with D_ia of both spins side by side in the compound index, without the sqrt(2) of the restricted singlets.
// tf_tddft_uhf is the same driver with xc set: the exchange blocks scaled by hfx (the two (ab|ij) not built when hfx = 0) and, unless the
// grid's functional is the null one, the spin-blocked K of xc_kernel_spin_build added in the assembly pass (counted in the assembly slot).
static int ucis_driver(tf_ctx *ctx, const char *who, const tf_ucis_opts *opts, const ExcXc *xc, int n_alpha, int n_beta, int n_frozen_alpha,
                       int n_frozen_beta, const double *C_alpha, const double *C_beta, const double *eps_alpha, const double *eps_beta, const double *dip,
                       tf_ucis_result *out)
{
    const std::string me = who;
    UcisSetup U;
    int rc = ucis_begin(ctx, who, opts && C_alpha && C_beta && eps_alpha && eps_beta && out, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, C_alpha, C_beta, U);
    if (rc) return rc;
    if (opts->n_keep < 0) TF_FAIL(ctx, TF_EINVAL, "%s: n_keep must not be negative", who);
    if ((out->tdm || out->osc) && !dip) TF_FAIL(ctx, TF_EINVAL, "%s: transition dipoles and oscillator strengths need the AO dipole matrices (dip)", who);
    if (xc && (rc = xc_kernel_checks(ctx, who, *xc, 2))) return rc;
    const double hfx = xc ? xc->hfx : 1.0;
    const bool with_k = xc && (ctx->grid.xid != 0 || ctx->grid.cid != 0);
    const int N = U.N, dim = U.dim, nk = std::min(opts->n_keep, dim);
    const size_t B2 = (size_t)dim * dim;
    const bool tda = opts->tda != 0, moments = dip && (out->tdm || out->osc);
    out->dim = dim; out->dim_alpha = (int)U.d[0];
    DeviceBlocks mem;
    tfucis::AssembleArgs A{};
    if ((rc = ucis_mo_blocks(ctx, who, U, mem, A, hfx != 0.0))) return rc;
    const auto t1 = corr_stamp();
    // ---- the exchange-correlation kernel matrix (TD-DFT)
    double *K = nullptr;
    if (with_k && (rc = xc_kernel_spin_build(ctx, who, U, xc->P[0], xc->P[1], mem, &K, nullptr))) return rc;
    // ---- work space: the matrices (CIS: A; TDHF: A + B and A - B) and the small arrays of the plan (C_o, C_v, D C_v of the larger spin)
    const ExcitedPlan P = excited_plan_uhf(N, dim, std::max(U.s[0].o, U.s[1].o), std::max(U.s[0].v, U.s[1].v), tda, nk);
    double *Mp = mem.alloc(B2), *Mm = tda ? nullptr : mem.alloc(B2), *small = mem.alloc(P.total);
    rocblas_int *d_info = mem.alloc_int(4);
    if (!Mp || (!tda && !Mm) || !small || !d_info) return exc_work_oom(ctx, who, P, "(d_alpha + d_beta)");
    // ---- assembly
    A.kind[0] = tda ? 0 : 1; A.out[0] = Mp; A.n_out = 1;
    if (!tda) { A.kind[1] = 2; A.out[1] = Mm; A.n_out = 2; }
    A.hfx = hfx; A.K = K; A.kfac[0] = tda ? 1.0 : 2.0;           // A gains K, A + B gains 2 K, A - B nothing
    if ((rc = ucis_assemble(ctx, who, U, mem, A, eps_alpha, eps_beta, P.at(small, EXC_EPS)))) return rc;
    mem.release(K);
    if ((out->m_plus && hipMemcpy(out->m_plus, Mp, B2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (out->m_minus && Mm && hipMemcpy(out->m_minus, Mm, B2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
        return corr_fail(ctx, TF_ENODEVICE, me + ": copy failed");
    const auto t2 = corr_stamp();
    // ---- solves
    CisSolve sv;
    if ((rc = cis_solve_begin(sv, ctx, who, "UHF", P, small, d_info, mem))) return rc;
    BlasAtomicsOff no_atomics(sv.blas);                       // no atomics in the products: split-K sums would change from run to run
    if (moments && (rc = cis_dipoles(sv, P, small, N, dip, 2, U.s, U.d))) return rc;
    if (tda) {
        if ((rc = cis_tda_solve(sv, Mp, "unrestricted", out->x, out->y))) return rc;
    } else {
        if ((rc = cis_tdhf_factor(sv, Mm, ""))) return rc;
        if ((rc = cis_tdhf_solve(sv, Mm, Mp, "spin-conserving", out->x, out->y))) return rc;
    }
    if (out->e && hipMemcpy(out->e, sv.d_w, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, me + ": copy failed");
    // mu_n[c] = sum over both spins of D^c_ia V[ia][n]: no sqrt(2)
    if (moments && (rc = cis_transition_moments(sv, P, small, tda ? Mp : sv.T, 1.0, out->tdm, out->osc))) return rc;
    if (hipGetLastError() != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, me + ": a kernel launch failed");
    corr_stage_seconds(out->seconds, U.t0, t1, t2, corr_stamp());
    return TF_OK;
}

int tf_cis_uhf(tf_ctx *ctx, const tf_ucis_opts *opts, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha,
               const double *C_beta, const double *eps_alpha, const double *eps_beta, const double *dip, tf_ucis_result *out)
{
    return ucis_driver(ctx, "tf_cis_uhf", opts, nullptr, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, C_alpha, C_beta, eps_alpha, eps_beta, dip, out);
}

int tf_tddft_uhf(tf_ctx *ctx, const tf_utddft_opts *opts, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha,
                 const double *C_beta, const double *eps_alpha, const double *eps_beta, const double *P_alpha, const double *P_beta, const double *dip,
                 tf_ucis_result *out)
{
    tf_ucis_opts uo{};
    ExcXc xc;
    if (opts) { uo.tda = opts->tda; uo.n_keep = opts->n_keep; xc.hfx = opts->hfx; }
    xc.P[0] = P_alpha; xc.P[1] = P_beta;
    return ucis_driver(ctx, "tf_tddft_uhf", opts ? &uo : nullptr, &xc, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, C_alpha, C_beta, eps_alpha, eps_beta,
                       dip, out);
}

// The solves of the stability analysis: the eigenvalues of each of the n matrices M[k] (order dim) to spec[k][dim] on the host and -- when
// the mode is asked for -- the eigenvector of each matrix's lowest eigenvalue to vec0[k][dim]; then the verdict:
// lowest[k] = min(l_min(plus[k]), l_min(minus)) with its source and mode; ties go to A + B
static int stability_solves(tf_ctx *ctx, const char *who, const ExcitedPlan &P, double *small, rocblas_int *d_info, int n, double *const *M,
                            const int plus[2], int minus, tf_stability_result *out)
{
    rocblas_handle blas = ctx->scf.blas;
    BlasAtomicsOff no_atomics(blas);
    const int dim = P.dim;
    const bool vectors = out->kappa != nullptr;
    double *d_w = P.at(small, EXC_W), *d_e = P.at(small, EXC_E);
    std::vector<double> spec((size_t)n * dim, 0.0), vec0(vectors ? (size_t)n * dim : 0, 0.0);
    for (int k = 0; k < n; ++k) {
        CIS_BLAS(rocsolver_dsyevd(blas, vectors ? rocblas_evect_original : rocblas_evect_none, rocblas_fill_upper, dim, M[k], dim, d_w, d_e, d_info));
        int h = 0;
        if (hipMemcpy(&h, d_info, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": the eigensolver failed on the device");
        if (h != 0) return corr_fail(ctx, TF_ELINALG, std::string(who) + ": the eigenvalues of an orbital-rotation matrix did not converge (rocsolver_dsyevd)");
        if (hipMemcpy(spec.data() + (size_t)k * dim, d_w, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            (vectors && hipMemcpy(vec0.data() + (size_t)k * dim, M[k], (size_t)dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
            return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    }
    for (int k = 0; k < 2; ++k) {
        const double lp = spec[(size_t)plus[k] * dim], lm = spec[(size_t)minus * dim];
        const int src = lm < lp ? minus : plus[k];
        out->lowest[k] = spec[(size_t)src * dim];
        out->source[k] = src;
        if (out->kappa) std::copy(vec0.begin() + (size_t)src * dim, vec0.begin() + (size_t)(src + 1) * dim, out->kappa + (size_t)k * dim);
    }
    if (out->spectra) std::copy(spec.begin(), spec.end(), out->spectra);
    return TF_OK;
}

// RHF stability (tuna_ci.py:926-985): tf_cis_rhf's MO blocks and assembly pass with kinds 2, 3, 4, then three dsyevd
// tf_stability_rks is the same driver with xc set (tuna_ci.py:1049-1106): the exchange blocks scaled by hfx ((ab|ij) not built when
// hfx = 0), 2 K_S added to the singlet A + B and 2 K_T to the triplet A + B (xc_kernel_build); A - B carries no kernel.
static int stability_restricted(tf_ctx *ctx, const char *who, const ExcXc *xc, int n_occ, int n_frozen, const double *C, const double *eps,
                                tf_stability_result *out)
{
    int rc = corr_args(ctx, who, C && eps && out, " (needs C, eps, out and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    if (xc && (rc = xc_kernel_checks(ctx, who, *xc, 1))) return rc;
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const long long B2 = S.B2;
    if (S.ov > 2000000LL || (long long)S.v * S.v > 2000000LL) TF_FAIL(ctx, TF_EINVAL, "%s: dimension overflow", who);
    const int dim = (int)S.ov;
    out->dim = dim; out->dim_alpha = dim; out->n_matrices = 3;
    DeviceBlocks mem;
    CisBlocks B;
    if ((rc = cis_mo_blocks(ctx, who, S, xc, mem, B))) return rc;
    const ExcitedPlan P = excited_plan_stability(S.N, dim, 1);
    double *M[3] = {mem.alloc((size_t)B2), mem.alloc((size_t)B2), mem.alloc((size_t)B2)}, *small = mem.alloc(P.total);
    rocblas_int *d_info = mem.alloc_int(4);
    if ((B.g2 && !B.Ht) || !M[0] || !M[1] || !M[2] || !small || !d_info) return exc_work_oom(ctx, who, P, "(o v)");
    const CisMatrix Ms[3] = {{2, B.KS, 2.0, M[0]}, {3, B.KT, 2.0, M[1]}, {4, nullptr, 0.0, M[2]}};     // A + B gains 2 K, A - B nothing
    if ((rc = cis_assemble(ctx, who, S, mem, B, eps, P.at(small, EXC_EPS), Ms, 3))) return rc;
    const auto t2 = corr_stamp();
    const int plus[2] = {0, 1};
    if ((rc = stability_solves(ctx, who, P, small, d_info, 3, M, plus, 2, out))) return rc;
    corr_stage_seconds(out->seconds, S.t0, B.t1, t2, corr_stamp());
    return TF_OK;
}

int tf_stability_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, tf_stability_result *out)
{
    return stability_restricted(ctx, "tf_stability_rhf", nullptr, n_occ, n_frozen, C, eps, out);
}

int tf_stability_rks(tf_ctx *ctx, double hfx, int n_occ, int n_frozen, const double *C, const double *eps, const double *P, tf_stability_result *out)
{
    const ExcXc xc{hfx, {P, nullptr}};
    return stability_restricted(ctx, "tf_stability_rks", &xc, n_occ, n_frozen, C, eps, out);
}

// UHF stability (tuna_ci.py:994-1038; the spin-conserving Hessian of build_orbital_hessian): tf_cis_uhf's blocks and assembly pass with
// A + B and A - B, then two dsyevd.  tf_stability_uks is the same driver with xc set: the exchange blocks scaled by hfx and 2 K of
// xc_kernel_spin_build added to A + B.
static int stability_unrestricted(tf_ctx *ctx, const char *who, const ExcXc *xc, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta,
                                  const double *C_alpha, const double *C_beta, const double *eps_alpha, const double *eps_beta, tf_stability_result *out)
{
    UcisSetup U;
    int rc = ucis_begin(ctx, who, C_alpha && C_beta && eps_alpha && eps_beta && out, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, C_alpha, C_beta, U);
    if (rc) return rc;
    if (xc && (rc = xc_kernel_checks(ctx, who, *xc, 2))) return rc;
    const double hfx = xc ? xc->hfx : 1.0;
    const bool with_k = xc && (ctx->grid.xid != 0 || ctx->grid.cid != 0);
    const int dim = U.dim;
    const size_t B2 = (size_t)dim * dim;
    out->dim = dim; out->dim_alpha = (int)U.d[0]; out->n_matrices = 2;
    DeviceBlocks mem;
    tfucis::AssembleArgs A{};
    if ((rc = ucis_mo_blocks(ctx, who, U, mem, A, hfx != 0.0))) return rc;
    const auto t1 = corr_stamp();
    double *K = nullptr;
    if (with_k && (rc = xc_kernel_spin_build(ctx, who, U, xc->P[0], xc->P[1], mem, &K, nullptr))) return rc;
    const ExcitedPlan P = excited_plan_stability(U.N, dim, 2);
    double *M[2] = {mem.alloc(B2), mem.alloc(B2)}, *small = mem.alloc(P.total);
    rocblas_int *d_info = mem.alloc_int(4);
    if (!M[0] || !M[1] || !small || !d_info) return exc_work_oom(ctx, who, P, "(d_alpha + d_beta)");
    A.n_out = 2; A.kind[0] = 1; A.out[0] = M[0]; A.kind[1] = 2; A.out[1] = M[1];
    A.hfx = hfx; A.K = K; A.kfac[0] = 2.0;                       // A + B gains 2 K, A - B nothing
    if ((rc = ucis_assemble(ctx, who, U, mem, A, eps_alpha, eps_beta, P.at(small, EXC_EPS)))) return rc;
    mem.release(K);
    const auto t2 = corr_stamp();
    const int plus[2] = {0, 0};
    if ((rc = stability_solves(ctx, who, P, small, d_info, 2, M, plus, 1, out))) return rc;
    corr_stage_seconds(out->seconds, U.t0, t1, t2, corr_stamp());
    return TF_OK;
}

int tf_stability_uhf(tf_ctx *ctx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha, const double *C_beta,
                     const double *eps_alpha, const double *eps_beta, tf_stability_result *out)
{
    return stability_unrestricted(ctx, "tf_stability_uhf", nullptr, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, C_alpha, C_beta, eps_alpha, eps_beta, out);
}

int tf_stability_uks(tf_ctx *ctx, double hfx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha, const double *C_beta,
                     const double *eps_alpha, const double *eps_beta, const double *P_alpha, const double *P_beta, tf_stability_result *out)
{
    const ExcXc xc{hfx, {P_alpha, P_beta}};
    return stability_unrestricted(ctx, "tf_stability_uks", &xc, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, C_alpha, C_beta, eps_alpha, eps_beta, out);
}
#undef CIS_BLAS

// CIS(D) of closed-shell CIS / TDHF states (calculate_restricted_doubles_correction, tuna_ci.py:1874-1982; tf_cisd.hip.h has the
// expressions and the kernels).  Stages: (ia|jb) and (ik|jb) through mo_transform_device, t, tt and L in one pass, Goo and Gvv by one GEMM
// each; then state by state the dressed block (i~ a|jb) through mo_transform_device with Ct_o = C_v b^T made on the device, the (ik|jb)
// GEMMs that turn it into M, the fused direct kernel, and the matrix-vector products of the indirect part.  Every state goes through
// the same calls with the same shapes whatever else the call holds, so its numbers do not depend on its neighbours; states do not share
// a transformation or a GEMM (rocBLAS promises the same bits for the same call, not for one column of a wider one).
// Work space: 5 arrays of o^2 v^2 (g, t, tt, L, M) and on the packed and tiles layouts 2 more inside a transformation.
int tf_cis_d_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, int n_states, const double *b, const double *omega,
                 const int32_t *triplet, tf_cis_d_result *out)
{
    static const char *who = "tf_cis_d_rhf";
    const bool pointers = C && eps && b && omega && triplet && out && out->e_d && out->e_direct && out->e_indirect;
    int rc = corr_args(ctx, who, pointers, " (needs C, eps, b, omega, triplet, out with e_d, e_direct and e_indirect, and 0 <= n_frozen < n_occ < N)",
                       n_occ, n_frozen);
    if (rc) return rc;
    if (n_states < 1) TF_FAIL(ctx, TF_EINVAL, "tf_cis_d_rhf: n_states must be at least 1, got %d", n_states);
    for (int s = 0; s < n_states; ++s)
        if (triplet[s] != 0 && triplet[s] != 1) TF_FAIL(ctx, TF_EINVAL, "tf_cis_d_rhf: triplet[%d] = %d is neither 0 (singlet) nor 1 (triplet)", s, (int)triplet[s]);
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const int N = S.N, o = S.o, v = S.v;
    const long long ov = S.ov, B2 = S.B2, nblk = tfcisd::tile_blocks(o, v);
    if (ov > 0x7fffffffLL / std::max(o, v) || nblk > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tf_cis_d_rhf: dimension overflow");
    const int dim = (int)ov;
    DeviceBlocks mem;
    auto fail = [&](int code, const std::string &m) { return corr_fail(ctx, code, m); };
    auto oom = [&](const char *what, size_t doubles) {
        char text[240];
        snprintf(text, sizeof text, "tf_cis_d_rhf: out of device memory for %.2f GB of %s (5 arrays of (o v)^2 = %lld^2 values in all)",
                 (double)doubles * sizeof(double) / 1e9, what, ov);
        return fail(TF_ENOMEM, text);
    };
    // ---- state-independent blocks: g = (ia|jb), h[i][k][j][b] = (ik|jb) = (ki|jb)
    double *g = nullptr, *h = nullptr;
    if ((rc = mo_transform_device(ctx, S.Co.data(), o, S.Cv.data(), v, S.Co.data(), o, S.Cv.data(), v, mem, &g, nullptr)))
        return rc == TF_ENOMEM ? oom("the transformation to (ia|jb)", 3 * (size_t)B2) : rc;
    if ((rc = mo_transform_device(ctx, S.Co.data(), o, S.Co.data(), o, S.Co.data(), o, S.Cv.data(), v, mem, &h, nullptr)))
        return rc == TF_ENOMEM ? oom("the transformation to (ki|jb)", 3 * (size_t)o * o * dim) : rc;
    // t | tt | L, and the small arrays: eps [N] | C_v [N][v] | Ct_o [N][o] | b [o][v] | x [dim] | y [dim] | Goo [o][o] | Gvv [v][v]
    const size_t nsmall = (size_t)N + (size_t)N * v + (size_t)N * o + 3 * (size_t)dim + (size_t)o * o + (size_t)v * v;
    double *ops = mem.alloc(3 * (size_t)B2);
    if (!ops) return oom("operands", 3 * (size_t)B2);
    double *small = mem.alloc(nsmall), *d_part = mem.alloc(2 * (size_t)nblk);
    if (!small || !d_part) return oom("partial sums", nsmall + 2 * (size_t)nblk);
    double *t = ops, *tt = t + B2, *L = tt + B2;
    double *d_eps = small, *d_Cv = d_eps + N, *d_Ct = d_Cv + (size_t)N * v, *d_b = d_Ct + (size_t)N * o, *d_x = d_b + dim, *d_y = d_x + dim, *d_Goo = d_y + dim,
           *d_Gvv = d_Goo + (size_t)o * o, *d_pmin = d_part + nblk;
    if (hipMemcpy(d_eps, eps, (size_t)N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_Cv, S.Cv.data(), (size_t)N * v * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(TF_ENODEVICE, "tf_cis_d_rhf: copy failed");
    rocblas_handle blas = ctx->scf.blas;
    BlasAtomicsOff no_atomics(blas);                          // no split-K sums: the same call gives the same bits
    tfcisd::launch_operands(g, d_eps, n_frozen, n_occ, o, v, t, tt, L, 0);
    // Goo[i][j] = sum_(bkc) t[i][(bkc)] L[j][(bkc)];  Gvv[b][a] = sum_(kcj) L[(kcj)][b] t[(kcj)][a]  (t and L are symmetric in their pairs)
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, o, o, v * dim, 1.0, t, v * dim, L, v * dim, 0.0, d_Goo, o));
    CORR_BLAS(tfmp3::gemm_rm(blas, true, false, v, v, o * dim, 1.0, L, v, t, v, 0.0, d_Gvv, v));
    std::vector<double> Goo((size_t)o * o), Gvv((size_t)v * v), y((size_t)dim), pmin((size_t)nblk);
    if (hipMemcpy(Goo.data(), d_Goo, Goo.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(Gvv.data(), d_Gvv, Gvv.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
        return fail(TF_ENODEVICE, "tf_cis_d_rhf: the operand kernel or the GEMMs of the intermediates failed on the device");
    const auto t1 = corr_stamp();
    std::chrono::steady_clock::duration d_transform{}, d_rest{};
    // y = alpha A x + beta y for a row-major A [dim][dim]
    auto matvec = [&](double alpha, const double *A, const double *x, double beta, double *yv) {
        return rocblas_dgemv(blas, rocblas_operation_transpose, dim, dim, &alpha, A, dim, x, 1, &beta, yv, 1);
    };
    std::vector<double> Ct((size_t)N * o);
    for (int s = 0; s < n_states; ++s) {
        const double *bs = b + (size_t)s * dim;
        const auto ta = corr_stamp();
        // ---- Ct_o = C_v b^T [N][o], and the dressed block (i~ a|j b)
        if (hipMemcpy(d_b, bs, (size_t)dim * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(TF_ENODEVICE, "tf_cis_d_rhf: copy failed");
        CORR_BLAS(tfmp3::gemm_rm(blas, false, true, N, o, v, 1.0, d_Cv, v, d_b, v, 0.0, d_Ct, o));
        if (hipMemcpy(Ct.data(), d_Ct, Ct.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(TF_ENODEVICE, "tf_cis_d_rhf: copy failed");
        DeviceBlocks state;                                   // M: gone before the next state's transformation
        double *M = nullptr;
        if ((rc = mo_transform_device(ctx, Ct.data(), o, S.Cv.data(), v, S.Co.data(), o, S.Cv.data(), v, state, &M, nullptr)))
            return rc == TF_ENOMEM ? oom("the dressed transformation", 3 * (size_t)B2) : rc;
        const auto tb = corr_stamp();
        // ---- M[i][a][(jb)] -= sum_k b[k][a] h[i][k][(jb)]
        CORR_BLAS(tfmp3::gemm_rm_batched(blas, true, false, v, dim, o, -1.0, d_b, v, 0, h, dim, (long long)o * dim, 1.0, M, dim, (long long)v * dim, o));
        tfcisd::launch_direct(M, d_eps, n_frozen, n_occ, o, v, omega[s], triplet[s], d_part, d_pmin, 0);
        double e_direct = 0.0;
        if (sum_partials_host(d_part, (int)nblk, 1, &e_direct) != hipSuccess ||
            hipMemcpy(pmin.data(), d_pmin, (size_t)nblk * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(TF_ENODEVICE, "tf_cis_d_rhf: the direct kernel failed on the device");
        double dmin = INFINITY;
        for (long long k = 0; k < nblk; ++k) dmin = std::min(dmin, pmin[(size_t)k]);
        // ---- x = L b, y = tt x (singlet);  x = (2 g - L) b, y = (2 t - tt) x (triplet)
        if (triplet[s]) {
            CORR_BLAS(matvec(2.0, g, d_b, 0.0, d_x));
            CORR_BLAS(matvec(-1.0, L, d_b, 1.0, d_x));
            CORR_BLAS(matvec(2.0, t, d_x, 0.0, d_y));
            CORR_BLAS(matvec(-1.0, tt, d_x, 1.0, d_y));
        } else {
            CORR_BLAS(matvec(1.0, L, d_b, 0.0, d_x));
            CORR_BLAS(matvec(1.0, tt, d_x, 0.0, d_y));
        }
        if (hipMemcpy(y.data(), d_y, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
            return fail(TF_ENODEVICE, "tf_cis_d_rhf: the products of the indirect part failed on the device");
        double e_y = 0.0, e_oo = 0.0, e_vv = 0.0;
        for (int k = 0; k < dim; ++k) e_y += bs[k] * y[(size_t)k];
        for (int i = 0; i < o; ++i)
            for (int j = 0; j < o; ++j) {
                double bb = 0.0;
                for (int a = 0; a < v; ++a) bb += bs[(size_t)i * v + a] * bs[(size_t)j * v + a];
                e_oo += bb * Goo[(size_t)i * o + j];
            }
        for (int c = 0; c < v; ++c)
            for (int a = 0; a < v; ++a) {
                double bb = 0.0;
                for (int i = 0; i < o; ++i) bb += bs[(size_t)i * v + a] * bs[(size_t)i * v + c];
                e_vv += bb * Gvv[(size_t)c * v + a];
            }
        out->e_direct[s] = e_direct;
        out->e_indirect[s] = (e_y - e_oo) - e_vv;
        out->e_d[s] = out->e_direct[s] + out->e_indirect[s];
        if (out->min_denominator) out->min_denominator[s] = dmin;
        const auto tc = corr_stamp();
        d_transform += tb - ta;
        d_rest += tc - tb;
    }
    out->seconds[0] = corr_secs(t1 - S.t0);
    out->seconds[1] = corr_secs(d_transform);
    out->seconds[2] = corr_secs(d_rest);
    return TF_OK;
}
