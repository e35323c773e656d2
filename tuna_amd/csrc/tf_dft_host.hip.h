// tf_dft_host.hip.h -- the host side of the Kohn-Sham path: the grid's two buffer sets through their owner, the grid precondition of
// every consumer, the density stages and the V assembly that the restricted and the unrestricted V_XC share (the density stages also
// with the kernel builds of tf_excited_host.hip.h, included after this file), and the four tf_dft_* entry points.  Included by
// tf_device.hip (one translation unit: struct tf_ctx, TF_FAIL, HIPCHK and sum_partials_host are defined there, above the include).
// Kernels and functional formulas: tf_dft.hip.h; buffer lists, lengths and the split: tf_dft_plan.h.  DESIGN.md section 4.6d.  Every
// launch, rocBLAS call and copy is on the null stream, in the order it always had.
#pragma once

namespace tfdft {

static inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? TF_ENOMEM : TF_ENODEVICE; }
// (both need `msg` in scope)
#define TFD_HIP(call) do { hipError_t _e = (call); if (_e != hipSuccess) { msg = std::string(#call) + " failed: " + hipGetErrorString(_e); return tfdft::hip_code(_e); } } while (0)
#define TFD_BLAS(call) do { rocblas_status _s = (call); if (_s != rocblas_status_success) { msg = std::string(#call) + " failed (rocBLAS status " + std::to_string((int)_s) + ")"; return TF_ELINALG; } } while (0)

// The grid's blocks come from the runtime's own hipMalloc / hipFree: they bypass tf_ctx.hip.h's small-block cache on purpose
static int grid_alloc(void **p, size_t bytes) { return (int)::hipMalloc(p, bytes); }
static void grid_free(void *p) { (void)::hipFree(p); }

// The spin set, whole or not at all, at the first unrestricted use of a grid
inline int ensure_spin(Grid &g, std::string &msg)
{
    if (g.spin.held()) return TF_OK;
    size_t len[GS_COUNT];
    grid_spin_lengths(g.G, g.N, len);
    hipError_t e = (hipError_t)g.spin.acquire(len, GS_COUNT, grid_alloc, grid_free);
    if (e != hipSuccess) { msg = std::string("unrestricted V_XC buffers: hipMalloc failed: ") + hipGetErrorString(e); return hip_code(e); }
    if (!g.gga && (e = hipMemset(g.s(GS_PT), 0, len[GS_PT] * sizeof(double))) != hipSuccess) {   // (LDA: the gradient rows stay zero)
        g.spin.release();
        msg = std::string("unrestricted V_XC buffers: hipMemset failed: ") + hipGetErrorString(e);
        return hip_code(e);
    }
    return TF_OK;
}

// ---- the stages V_XC shares with the exchange-correlation kernel builds (which pass gga = 0: they run on local-density grids only) ----

// Restricted: B (G x N, row-major) = Phi (G x N) * P (N x N), then rho and -- gga -- 2 grad rho of every point from B.  (This GEMM is the
// rocblas_dgemm call that tfmp3::gemm_rm(blas, false, false, G, N, N, 1.0, phi, N, P, N, 0.0, B, N) makes: same operations, sizes, operands.)
inline rocblas_status density_stage(rocblas_handle blas, const Grid &g, const double *dP, int gga)
{
    const int N = g.N;
    const long long G = g.G;
    const double one = 1.0, zero = 0.0;
    const rocblas_status s = rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_none, N, (rocblas_int)G, N, &one, dP, N, g.b(GB_PHI), N, &zero,
                                           g.b(GB_B), N);
    if (s != rocblas_status_success) return s;
    hipLaunchKernelGGL(xc_density_kernel, dim3((unsigned)((G + 15) / 16)), dim3(256), 0, 0, G, N, g.b(GB_PHI), g.b(GB_DPHI), g.b(GB_B), gga, g.b(GB_RHO),
                       g.b(GB_GRAD));
    return s;
}

// Both spins: [P_a | P_b] packed, B2 (G x 2N, row-major) = Phi (G x N) * [P_a | P_b] (N x 2N), then rows 0-7 of pt.  Needs the spin set.
inline rocblas_status density2_stage(rocblas_handle blas, const Grid &g, const double *dPa, const double *dPb, int gga)
{
    const int N = g.N, N2 = 2 * g.N;
    const long long G = g.G;
    const double one = 1.0, zero = 0.0;
    hipLaunchKernelGGL(pack2_kernel, dim3((unsigned)((2 * (size_t)N * N + 255) / 256)), dim3(256), 0, 0, dPa, dPb, g.s(GS_P), N);
    const rocblas_status s = rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_none, N2, (rocblas_int)G, N, &one, g.s(GS_P), N2, g.b(GB_PHI), N,
                                           &zero, g.s(GS_B), N2);
    if (s != rocblas_status_success) return s;
    hipLaunchKernelGGL(xc_density2_kernel, dim3((unsigned)((G + 15) / 16)), dim3(256), 0, 0, G, N, g.b(GB_PHI), g.b(GB_DPHI), g.s(GS_B), gga, g.s(GS_PT));
    return s;
}

// ---- V = Phi^T D, split over the grid points -------------------------------------------------------------------------------------

// (N x ldD, row-major) = Phi^T (N x G) * D (G x ldD) by the parts of S (S.width = N ldD) into V's slots, then their sum in part order
// into the sum slot: ldD = N for the restricted D, 2N for both spins side by side
inline rocblas_status v_assemble(rocblas_handle blas, const Grid &g, const double *D, int ldD, double *V, const SplitPlan &S)
{
    const int N = g.N;
    const double one = 1.0, zero = 0.0;
    const double *phi = g.b(GB_PHI);
    rocblas_status s = rocblas_status_success;
    if (S.Kc > 0)
        s = rocblas_dgemm_strided_batched(blas, rocblas_operation_none, rocblas_operation_transpose, ldD, N, (rocblas_int)S.Kc, &one, D, ldD,
                                          (rocblas_stride)(S.Kc * ldD), phi, N, (rocblas_stride)(S.Kc * N), &zero, V, ldD, (rocblas_stride)S.width, VSPLIT);
    if (s == rocblas_status_success && S.rem > 0)
        s = rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_transpose, ldD, N, (rocblas_int)S.rem, &one, D + S.first_rem * ldD, ldD,
                          phi + S.first_rem * N, N, &zero, V + S.part_off(S.rem_slot), ldD);
    if (s != rocblas_status_success) return s;
    hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((S.width + 255) / 256)), dim3(256), 0, 0, V, S.nparts, V + S.sum_off(), (int)S.width);
    return s;
}

// V_XC (device, [N][N]) and the integrals {n_elec, E_X*dfx, E_C*dfc} for the device density dP
inline int vxc(rocblas_handle blas, Grid &g, const double *dP, double *dVxc, double out3[3], std::string &msg)
{
    const int N = g.N, gga = g.gga ? 1 : 0;
    const long long G = g.G;
    TFD_BLAS(density_stage(blas, g, dP, gga));
    hipLaunchKernelGGL(xc_point_kernel, dim3((unsigned)((G + 127) / 128)), dim3(128), 0, 0, G, gga, g.xid, g.cid, g.dfx, g.dfc, g.x_alpha, g.b(GB_RHO),
                       g.b(GB_GRAD), g.b(GB_VRHO), g.b(GB_VSIG), g.b(GB_EX), g.b(GB_EC));
    hipLaunchKernelGGL(xc_dmat_kernel, dim3((unsigned)((G * N + 255) / 256)), dim3(256), 0, 0, G, N, g.b(GB_W), g.b(GB_PHI), g.b(GB_DPHI), g.b(GB_GRAD),
                       g.b(GB_VRHO), g.b(GB_VSIG), gga, g.b(GB_D));
    const SplitPlan S = split_plan(G, (long long)N * N);
    TFD_BLAS(v_assemble(blas, g, g.b(GB_D), N, g.b(GB_V), S));
    hipLaunchKernelGGL(sym_kernel, dim3((N * N + 255) / 256), dim3(256), 0, 0, g.b(GB_V) + S.sum_off(), dVxc, N);
    hipLaunchKernelGGL(xc_reduce_kernel, dim3(NPART), dim3(256), 0, 0, G, g.b(GB_W), g.b(GB_RHO), g.b(GB_EX), g.b(GB_EC), g.b(GB_PART));
    TFD_HIP(sum_partials_host(g.b(GB_PART), NPART, 3, out3));
    out3[1] *= g.dfx; out3[2] *= g.dfc;
    return TF_OK;
}

// V_XC^alpha, V_XC^beta (device, [N][N]) and {n_alpha, n_beta, E_X,alpha*DFX, E_X,beta*DFX, E_C*DFC} for the device densities dPa, dPb
inline int vxc_unrestricted(rocblas_handle blas, Grid &g, const double *dPa, const double *dPb, double *dVa, double *dVb, double out5[5],
                            std::string &msg)
{
    int rc = ensure_spin(g, msg);
    if (rc) return rc;
    const int N = g.N, gga = g.gga ? 1 : 0;
    const long long G = g.G;
    TFD_BLAS(density2_stage(blas, g, dPa, dPb, gga));
    hipLaunchKernelGGL(xc_point2_kernel, dim3((unsigned)((G + 127) / 128)), dim3(128), 0, 0, G, gga, g.xid, g.cid, g.dfx, g.dfc, g.x_alpha, g.s(GS_PT));
    hipLaunchKernelGGL(xc_dmat2_kernel, dim3((unsigned)((G * N + 255) / 256)), dim3(256), 0, 0, G, N, g.b(GB_W), g.b(GB_PHI), g.b(GB_DPHI), g.s(GS_PT), gga,
                       g.s(GS_D));
    // [N][2N] = (Phi^T D2)^T: row j holds column j of both spins' products
    const SplitPlan S = split_plan(G, 2LL * N * N);
    TFD_BLAS(v_assemble(blas, g, g.s(GS_D), 2 * N, g.s(GS_V), S));
    hipLaunchKernelGGL(sym2_kernel, dim3((unsigned)((S.width + 255) / 256)), dim3(256), 0, 0, g.s(GS_V) + S.sum_off(), dVa, dVb, N);
    hipLaunchKernelGGL(xc_reduce5_kernel, dim3(NPART), dim3(256), 0, 0, G, g.b(GB_W), g.s(GS_PT), g.s(GS_PART));
    TFD_HIP(sum_partials_host(g.s(GS_PART), NPART, 5, out5));
    out5[2] *= g.dfx; out5[3] *= g.dfx; out5[4] *= g.dfc;
    return TF_OK;
}

}  // namespace tfdft

// ---- the grid precondition of every consumer --------------------------------------------------------------------------------------
// A grid (G > 0: tf_dft_setup commits a whole one or none) that was set up for this tensor.  Each caller keeps the wording it always
// had: `hint` follows "call tf_dft_setup first"; cycle: the wording of the SCF entry points for a grid of another AO dimension.
static int dft_grid_checks(tf_ctx *ctx, const char *who, const char *hint, bool cycle)
{
    if (ctx->grid.G <= 0) TF_FAIL(ctx, TF_EINVAL, "%s: call tf_dft_setup first%s", who, hint);
    if (ctx->have_eri && ctx->grid.N == ctx->N) return TF_OK;
    if (cycle) TF_FAIL(ctx, TF_EINVAL, "%s: the DFT grid was set up for a different AO dimension", who);
    TF_FAIL(ctx, TF_EINVAL, "%s: the grid was set up for a different tensor (call tf_build_eri, then tf_dft_setup again)", who);
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------

int tf_dft_clear(tf_ctx *ctx)
{
    if (!ctx) return TF_EINVAL;
    (void)hipSetDevice(ctx->device);
    tfdft::release(ctx->grid);
    return TF_OK;
}

// Everything tf_dft_setup puts into a grid, into one the context does not see yet
static int dft_grid_build(tf_ctx *ctx, tfdft::Grid &g, int64_t n_points, const double *xyz, const double *weights, int x_functional, int c_functional,
                          double dfx, double dfc, double x_alpha)
{
    const int N = ctx->N;
    const long long G = n_points;
    g.G = G; g.N = N; g.xid = x_functional; g.cid = c_functional; g.dfx = dfx; g.dfc = dfc; g.x_alpha = x_alpha;
    g.gga = (x_functional >= tfdft::X_B88) || (c_functional >= tfdft::C_LYP);
    std::string err;
    tfone::DevBuf buf;
    tfone::DAO A = tfone::upload_aos(ctx->bs, buf, err);
    if (!err.empty()) TF_FAIL(ctx, TF_ENODEVICE, "%s", err.c_str());
    double *d_xyz = buf.alloc<double>((size_t)3 * G, err);
    if (!err.empty()) TF_FAIL(ctx, TF_ENOMEM, "%s", err.c_str());
    HIPCHK(ctx, hipMemcpy(d_xyz, xyz, (size_t)3 * G * sizeof(double), hipMemcpyHostToDevice));
    size_t len[tfdft::GB_COUNT];
    tfdft::grid_base_lengths(G, N, g.gga, len);
    const hipError_t e = (hipError_t)g.base.acquire(len, tfdft::GB_COUNT, tfdft::grid_alloc, tfdft::grid_free);
    if (e != hipSuccess) TF_FAIL(ctx, tfdft::hip_code(e), "tf_dft_setup: hipMalloc of the grid's buffers failed: %s", hipGetErrorString(e));
    HIPCHK(ctx, hipMemcpy(g.b(tfdft::GB_W), weights, (size_t)G * sizeof(double), hipMemcpyHostToDevice));
    tfdft::DAOs D{A.z, A.lmn, A.prim_off, A.exps, A.w};
    hipLaunchKernelGGL(tfdft::ao_on_grid_kernel, dim3((unsigned)((len[tfdft::GB_PHI] + 127) / 128)), dim3(128), 0, 0, D, d_xyz, G, N, ctx->d_csr_ptr(),
                       ctx->d_csr_idx(), ctx->d_csr_val(), g.b(tfdft::GB_PHI), g.b(tfdft::GB_DPHI), g.gga ? 1 : 0);
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipGetLastError());
    std::string msg;
    int rc = tfscf::ensure(ctx->scf, N, 6, msg);           // makes sure the rocBLAS handle exists
    if (rc) { ctx->err = msg; return rc; }
    return TF_OK;
}

int tf_dft_setup(tf_ctx *ctx, int64_t n_points, const double *xyz, const double *weights, int x_functional, int c_functional, double dfx,
                 double dfc, double x_alpha)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_dft_setup: call tf_build_eri first (it fixes the AO representation)");
    if (n_points < 1 || !xyz || !weights || x_functional < 0 || x_functional > 3 || c_functional < 0 || c_functional > 5)
        TF_FAIL(ctx, TF_EINVAL, "tf_dft_setup: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    tfdft::release(ctx->grid);                                  // (before the new grid is allocated: the two never coexist)
    tfdft::Grid fresh;
    const int rc = dft_grid_build(ctx, fresh, n_points, xyz, weights, x_functional, c_functional, dfx, dfc, x_alpha);
    if (rc) { tfdft::release(fresh); return rc; }              // the context is left without a grid: G == 0
    ctx->grid = fresh;
    return TF_OK;
}

// The density and V_XC are staged through the Fock build's own device buffers of one call, ctx->jk.all.P and .J ([N][N] each, allocated
// by every tensor build): tf_dft_vxc owns no staging buffer, and nothing else uses the two between its copies.
int tf_dft_vxc(tf_ctx *ctx, const double *P, double *Vxc, double *n_elec, double *e_x, double *e_c)
{
    if (!ctx) return TF_EINVAL;
    int rc = dft_grid_checks(ctx, "tf_dft_vxc", "", false);
    if (rc) return rc;
    if (!P || !Vxc) TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)ctx->N * ctx->N;
    HIPCHK(ctx, hipMemcpy(ctx->jk.all.P, P, nn * sizeof(double), hipMemcpyHostToDevice));
    std::string msg;
    double o3[3];
    rc = tfdft::vxc(ctx->scf.blas, ctx->grid, ctx->jk.all.P, ctx->jk.all.J, o3, msg);
    if (rc) { ctx->err = msg; return rc; }
    HIPCHK(ctx, hipMemcpy(Vxc, ctx->jk.all.J, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (n_elec) *n_elec = o3[0];
    if (e_x) *e_x = o3[1];
    if (e_c) *e_c = o3[2];
    return TF_OK;
}

int tf_dft_vxc_unrestricted(tf_ctx *ctx, const double *P_alpha, const double *P_beta, double *Vxc_alpha, double *Vxc_beta, double n_elec[2],
                            double e_x[2], double *e_c)
{
    if (!ctx) return TF_EINVAL;
    int rc = dft_grid_checks(ctx, "tf_dft_vxc_unrestricted", "", false);
    if (rc) return rc;
    if (!P_alpha || !P_beta || !Vxc_alpha || !Vxc_beta) TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc_unrestricted: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    rc = tfdft::ensure_spin(ctx->grid, msg);
    if (rc) { ctx->err = msg; return rc; }
    const size_t nn = (size_t)ctx->N * ctx->N;
    double *io = ctx->grid.s(tfdft::GS_IO);                      // P_alpha, P_beta, V_alpha, V_beta
    HIPCHK(ctx, hipMemcpy(io, P_alpha, nn * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(io + nn, P_beta, nn * sizeof(double), hipMemcpyHostToDevice));
    double o5[5];
    rc = tfdft::vxc_unrestricted(ctx->scf.blas, ctx->grid, io, io + nn, io + 2 * nn, io + 3 * nn, o5, msg);
    if (rc) { ctx->err = msg; return rc; }
    HIPCHK(ctx, hipMemcpy(Vxc_alpha, io + 2 * nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(Vxc_beta, io + 3 * nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (n_elec) { n_elec[0] = o5[0]; n_elec[1] = o5[1]; }
    if (e_x) { e_x[0] = o5[2]; e_x[1] = o5[3]; }
    if (e_c) *e_c = o5[4];
    return TF_OK;
}
