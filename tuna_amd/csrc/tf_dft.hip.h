// tf_dft.hip.h -- Kohn-Sham exchange-correlation on the GPU (BASELINE config 4: CO B3LYP/def2-TZVP).
// AOs and their gradients are evaluated once on the molecular grid; per SCF iteration the density, its gradient, the
// functional derivatives and the V_XC matrix are two GEMMs (rocBLAS) around element-wise kernels:
//     B = Phi P            rho_g = <B_g, Phi_g>     grad_a = 2 <B_g, dPhi_a,g>
//     D = w (vrho Phi + 4 vsigma sum_a grad_a dPhi_a)          V_XC = sym(Phi^T D)
// Reference: construct_basis_functions_on_grid tuna_dft.py:516-584, construct_basis_function_gradients_on_grid :586-666,
// construct_density_on_grid :677-703, calculate_density_gradient :714-744, calculate_V_X/V_C :788-888,
// calculate_restricted_exchange_correlation_matrix tuna_scf.py:600-654, functionals tuna_xc.py (Slater :199-213, B88 :385-438,
// B3 :1462-1494, VWN :1512-1630 + :1802-1860, LYP :2200-2260, 3P :5843-5881), floors tuna_util.py:95-99.
// For TD-DFT the second derivatives of the local-density functionals per grid point (xc_fpoint_kernel: Slater tuna_xc.py:5956-5983,
// VWN3 :5994-6061, VWN5 :6151-6236, the factors of tuna_dft.py:1109-1124); their matrix elements are tf_xckernel.hip.h's.
// Kernels and functional formulas only: the grid, its buffers and the split are tf_dft_plan.h's, every allocation and rocBLAS call
// tf_dft_host.hip.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "tf_dft_plan.h"

namespace tfdft {

enum { X_NONE = 0, X_SLATER = 1, X_B88 = 2, X_B3 = 3 };
enum { C_NONE = 0, C_VWN5 = 1, C_VWN3 = 2, C_LYP = 3, C_3P_VWN5 = 4, C_3P_VWN3 = 5 };

struct DAOs { const double *z; const int *lmn, *prim_off; const double *exps, *w; };

// phi[g][i], dphi[a][g][i] for OUTPUT AO i = sum over its CSR row of Cartesian AOs (identity row for Cartesian output)
__global__ void ao_on_grid_kernel(DAOs A, const double *__restrict__ xyz, long long G, int N, const int *__restrict__ ptr,
                                  const int *__restrict__ idx, const double *__restrict__ val, double *__restrict__ phi,
                                  double *__restrict__ dphi, int with_grad)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * N) return;
    const long long g = e / N;
    const int i = (int)(e - g * N);
    const double X = xyz[g], Y = xyz[G + g], Z = xyz[2 * G + g];
    double f = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
    for (int q = ptr[i]; q < ptr[i + 1]; ++q) {
        const int c = idx[q];
        const int l = A.lmn[3 * c], m = A.lmn[3 * c + 1], n = A.lmn[3 * c + 2];
        const double zr = Z - A.z[c];
        const double r2 = X * X + Y * Y + zr * zr;
        double px = 1.0, py = 1.0, pz = 1.0;
        for (int k = 0; k < l; ++k) px *= X;
        for (int k = 0; k < m; ++k) py *= Y;
        for (int k = 0; k < n; ++k) pz *= zr;
        double pxm = 1.0, pym = 1.0, pzm = 1.0;                 // x^(l-1), ...
        for (int k = 0; k + 1 < l; ++k) pxm *= X;
        for (int k = 0; k + 1 < m; ++k) pym *= Y;
        for (int k = 0; k + 1 < n; ++k) pzm *= zr;
        const double poly = px * py * pz;
        const double dpx = l > 0 ? l * pxm * py * pz : 0.0, dpy = m > 0 ? m * px * pym * pz : 0.0, dpz = n > 0 ? n * px * py * pzm : 0.0;
        double s = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        for (int p = A.prim_off[c]; p < A.prim_off[c + 1]; ++p) {
            const double a = A.exps[p];
            const double ew = A.w[p] * exp(-a * r2);
            s += ew;
            if (with_grad) {
                sx += ew * (dpx - 2.0 * a * X * poly);
                sy += ew * (dpy - 2.0 * a * Y * poly);
                sz += ew * (dpz - 2.0 * a * zr * poly);
            }
        }
        f += val[q] * s * poly;
        fx += val[q] * sx; fy += val[q] * sy; fz += val[q] * sz;
    }
    phi[e] = f;
    if (with_grad) { dphi[e] = fx; dphi[G * N + e] = fy; dphi[2 * G * N + e] = fz; }
}

// ---- functionals (restricted, closed shell) -------------------------------------------------------------------------

struct XcOut { double dfdn, dfds, e; };

__device__ inline XcOut slater_x(double n, double x_alpha)                     // tuna_xc.py:199-213
{
    XcOut o;
    o.dfdn = -(3.0 / 2.0 * x_alpha) * cbrt(3.0 / 3.141592653589793 * n);
    o.e = 3.0 / 4.0 * o.dfdn;
    o.dfds = 0.0;
    return o;
}

__device__ inline XcOut b88_x(double n, double sigma, double x_alpha)          // tuna_xc.py:385-438
{
    const double beta = 0.0042;
    const double C = 2.0 / cbrt(4.0);
    const double eLDA = slater_x(n / 2.0, x_alpha).e;
    const double c3 = cbrt(n / 2.0);
    const double x = sqrt(sigma / 4.0) / (c3 * c3 * c3 * c3);
    const double x2 = x * x;
    const double A = asinh(x);
    const double Dd = 1.0 + 6.0 * beta * x * A;
    const double D2 = Dd * Dd;
    const double dDdx = 6.0 * beta * (A + x / sqrt(1.0 + x2));
    XcOut o;
    o.e = C * eLDA - beta * c3 * x2 / Dd;
    o.dfdn = (o.e + C * eLDA / 3.0 + beta * c3 * (7.0 * x2 * Dd - 4.0 * x2 * x * dDdx) / (3.0 * D2));
    o.dfds = -beta * n * c3 * (x2 * Dd - (1.0 / 2.0) * x2 * x * dDdx) / (sigma * D2);
    return o;
}

__device__ inline XcOut vwn_c(double n, double x_0, double b, double c, double A)   // tuna_xc.py:1802-1860
{
    const double Q = sqrt(4.0 * c - b * b);
    const double X_0 = x_0 * x_0 + b * x_0 + c;
    const double c_1 = -b * x_0 / X_0;
    const double c_2 = 2.0 * b * (c - x_0 * x_0) / (Q * X_0);
    const double r_s = cbrt(3.0 / (4.0 * 3.141592653589793) * (1.0 / n));
    const double x = sqrt(r_s);
    const double xm = x - x_0;
    const double Xx = r_s + b * x + c;
    const double log1 = log(r_s / Xx);
    const double log2 = log(xm * xm / Xx);
    const double at = atan(Q / (2.0 * x + b));
    const double combo = (2.0 / x + 2.0 * c_1 / xm - (2.0 * x + b) * (1.0 + c_1) / Xx - (1.0 / 2.0) * c_2 * Q / Xx);
    XcOut o;
    o.e = A * (log1 + c_1 * log2 + c_2 * at);
    const double dedr = (A / 2.0) * combo / x;
    o.dfdn = o.e - r_s / 3.0 * dedr;
    o.dfds = 0.0;
    return o;
}

__device__ inline XcOut lyp_c(double n, double sigma)                           // tuna_xc.py:2200-2260
{
    const double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
    const double PI = 3.141592653589793;
    const double inv_n = 1.0 / n;
    const double c3 = cbrt(n);
    const double ic3 = 1.0 / c3;
    const double X = 1.0 + d * ic3;
    const double k = cbrt(3.0 * PI * PI);
    const double c3_2 = c3 * c3, c3_4 = c3_2 * c3_2, c3_8 = c3_4 * c3_4;
    const double C2 = 6.0 / 10.0 * k * k * c3_8;
    const double ic3_2 = ic3 * ic3, ic3_4 = ic3_2 * ic3_2, ic3_8 = ic3_4 * ic3_4;
    const double w = ic3_8 * ic3_2 * ic3 * exp(-c * ic3) / X;              // inv_cbrt^11
    const double delta = ic3 * (c + d / X);
    const double mabw = -a * b * w * n;
    const double wpw = -(1.0 / 3.0) * ic3_4 * (11.0 * c3 - c - d / X);
    const double dprime = (1.0 / 3.0) * (d * d * ic3_4 * ic3 / (X * X) - delta * inv_n);
    XcOut o;
    o.dfds = mabw * n * (-7.0 * delta - 3.0) / 72.0;
    double dfdn = -a / X + mabw * sigma * (-1.0 / 12.0 - 7.0 * delta / 36.0 + n * (-7.0 * dprime / 72.0 + wpw * (-1.0 / 24.0 - 7.0 * delta / 72.0)));
    dfdn += n * (-a * d / (3.0 * X * X * c3_4) - 7.0 * C2 * a * b * w / 3.0 - (1.0 / 2.0) * C2 * a * b * n * wpw * w);
    o.dfdn = dfdn;
    o.e = (1.0 / 2.0) * C2 * mabw - mabw * sigma * (7.0 * delta + 3.0) / 72.0 - a / X;
    return o;
}

// rho (raw) and 2 grad rho from B = Phi P: rho(g) = sum_i B[g][i] Phi[g][i], grad_a = 2 sum_i B[g][i] dPhi_a[g][i].  Sixteen lanes per grid
// point, each a sixteenth of the AOs (coalesced 128-byte reads of the point's rows; one thread per point walked its own row of every
// array with a stride of N doubles between neighbouring threads: 0.30 ms per call for CO / def2-TZVP, 3.6 ms of a 27 ms single point).
__global__ __launch_bounds__(256) void xc_density_kernel(long long G, int N, const double *__restrict__ phi, const double *__restrict__ dphi,
                                                         const double *__restrict__ B, int gga, double *__restrict__ rho, double *__restrict__ grad)
{
    const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
    const long long g = (long long)blockIdx.x * 16 + grp;
    double n = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    if (g < G) {
        const double *b = B + g * N, *f = phi + g * N;
        for (int i = l; i < N; i += 16) n += b[i] * f[i];
        if (gga) {
            const double *fx = dphi + g * N, *fy = dphi + G * N + g * N, *fz = dphi + 2 * G * N + g * N;
            for (int i = l; i < N; i += 16) { const double bi = b[i]; gx += bi * fx[i]; gy += bi * fy[i]; gz += bi * fz[i]; }
        }
    }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) {
        n += __shfl_xor(n, d, 16); gx += __shfl_xor(gx, d, 16); gy += __shfl_xor(gy, d, 16); gz += __shfl_xor(gz, d, 16);
    }
    if (l == 0 && g < G) {
        rho[g] = n;
        if (gga) { grad[g] = 2.0 * gx; grad[G + g] = 2.0 * gy; grad[2 * G + g] = 2.0 * gz; }
    }
}

// rho (floored), sigma (floored) of a point from xc_density_kernel's sums; then functional derivatives and energy densities
__global__ void xc_point_kernel(long long G, int gga, int xid, int cid, double dfx, double dfc, double x_alpha,
                                double *__restrict__ rho, const double *__restrict__ grad, double *__restrict__ vrho, double *__restrict__ vsig,
                                double *__restrict__ ex, double *__restrict__ ec)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double n = rho[g], gx = 0.0, gy = 0.0, gz = 0.0;
    if (gga) { gx = grad[g]; gy = grad[G + g]; gz = grad[2 * G + g]; }
    n = fmax(n, 1e-23);                                                     // xc.clean, density_floor
    const double sigma = fmax(gx * gx + gy * gy + gz * gz, 1e-46);          // sigma_floor
    XcOut X{0, 0, 0}, C{0, 0, 0};
    if (xid == X_SLATER) X = slater_x(n, x_alpha);
    else if (xid == X_B88) X = b88_x(n, sigma, x_alpha);
    else if (xid == X_B3) {                                                 // 0.9 B88 + 0.1 Slater, tuna_xc.py:1462-1494
        const XcOut s = slater_x(n, x_alpha), bb = b88_x(n, sigma, x_alpha);
        X.dfdn = 0.9 * bb.dfdn + 0.1 * s.dfdn; X.dfds = 0.9 * bb.dfds; X.e = 0.9 * bb.e + 0.1 * s.e;
    }
    if (cid == C_VWN5) C = vwn_c(n, -0.10498, 3.72744, 12.9352, 0.0310907);
    else if (cid == C_VWN3) C = vwn_c(n, -0.409286, 13.0720, 42.7198, 0.0310907);
    else if (cid == C_LYP) C = lyp_c(n, sigma);
    else if (cid == C_3P_VWN5 || cid == C_3P_VWN3) {                        // 0.81 LYP + 0.19 VWN, tuna_xc.py:5843-5881
        const XcOut l = (cid == C_3P_VWN5) ? vwn_c(n, -0.10498, 3.72744, 12.9352, 0.0310907) : vwn_c(n, -0.409286, 13.0720, 42.7198, 0.0310907);
        const XcOut y = lyp_c(n, sigma);
        C.dfdn = 0.81 * y.dfdn + 0.19 * l.dfdn; C.dfds = 0.81 * y.dfds; C.e = 0.81 * y.e + 0.19 * l.e;
    }
    rho[g] = n;
    vrho[g] = dfx * X.dfdn + dfc * C.dfdn;
    vsig[g] = dfx * X.dfds + dfc * C.dfds;
    ex[g] = X.e * n;
    ec[g] = C.e * n;
}

// ---- second functional derivatives of the local-density functionals: the exchange-correlation kernel of TD-DFT ------------------------
// (calculate_restricted_exchange_correlation_kernel_matrices, tuna_dft.py:1109-1124.)  With f = n e per functional,
//     f_X = 2 d2(n e_X)/dn2,   f_C^singlet = 2 d2(n e_C)/dn2,   f_C^triplet = 2 f_mm   (f_mm: the spin stiffness over the density)

__device__ inline double slater_d2f(double n, double x_alpha)                   // tuna_xc.py:5956-5983
{
    const double ic = 1.0 / cbrt(n);
    return -(x_alpha / 2.0) * cbrt(3.0 / 3.141592653589793) * ic * ic;
}

__device__ inline void vwn_pot(double n, double x_0, double b, double c, double A, double &e, double &dedr);   // (below, with the spin path)

struct VwnD2 { double e, dedr, d2edr2, r_s, x, combo, dcombo; };

__device__ inline VwnD2 vwn_d2(double n, double x_0, double b, double c, double A)   // tuna_xc.py:6247-6297
{
    const double Q = sqrt(4.0 * c - b * b);
    const double X_0 = x_0 * x_0 + b * x_0 + c;
    const double c_1 = -b * x_0 / X_0;
    const double c_2 = 2.0 * b * (c - x_0 * x_0) / (Q * X_0);
    VwnD2 o;
    o.r_s = cbrt(3.0 / (4.0 * 3.141592653589793) * (1.0 / n));
    o.x = sqrt(o.r_s);
    const double x = o.x, xm = x - x_0, Xx = o.r_s + b * x + c, X2 = Xx * Xx, xm2 = xm * xm;
    o.e = A * (log(o.r_s / Xx) + c_1 * log(xm2 / Xx) + c_2 * atan(Q / (2.0 * x + b)));
    o.combo = 2.0 / x + 2.0 * c_1 / xm - (2.0 * x + b) * (1.0 + c_1) / Xx - (1.0 / 2.0) * c_2 * Q / Xx;
    o.dcombo = (-2.0 / o.r_s - 2.0 * c_1 / xm2 - 2.0 * (1.0 + c_1) / Xx + ((2.0 * x + b) * (2.0 * x + b)) * (1.0 + c_1) / X2 +
                (1.0 / 2.0) * c_2 * Q * (2.0 * x + b) / X2);
    o.dedr = (A / 2.0) * o.combo / x;
    o.d2edr2 = A * (x * o.dcombo - o.combo) / (4.0 * x * x * x);
    return o;
}

// d2(n e_C)/dn2 and f_mm of VWN-III (tuna_xc.py:5994-6061) and VWN-V (:6151-6236)
__device__ inline void vwn3_kernel(double n, double &d2f, double &fmm)
{
    const VwnD2 p = vwn_d2(n, -0.409286, 13.0720, 42.7198, 0.0310907);
    d2f = (p.r_s * p.r_s * p.d2edr2 - 2.0 * p.r_s * p.dedr) / (9.0 * n);
    double e1, d1;
    vwn_pot(n, -0.743294, 20.1231, 101.578, 0.01554535, e1, d1);
    const double t = cbrt(2.0), fpp0 = 8.0 / (9.0 * (t * t * t * t - 2.0));
    fmm = fpp0 * (e1 - p.e) / n;
}
__device__ inline void vwn5_kernel(double n, double &d2f, double &fmm)
{
    const VwnD2 p = vwn_d2(n, -0.10498, 3.72744, 12.9352, 0.0310907);
    d2f = (p.x * 0.0310907) / (36.0 * n) * (p.x * p.dcombo - 5.0 * p.combo);
    double ma, dma;
    vwn_pot(n, -0.0047584, 1.13107, 13.0045, 1.0 / (6.0 * 3.141592653589793 * 3.141592653589793), ma, dma);
    fmm = -ma / n;
}

// rho (floored as in xc_point_kernel) of a point from xc_density_kernel's sum; the weights of the kernel matrices
//     u_S = w (dfx f_X + dfc f_C^S),   u_T = w (dfx f_X + dfc f_C^T);
// fpts (may be null): [4][G] = rho, f_X, f_C^S, f_C^T.  Local-density ids only (the caller refuses the others).
__global__ void xc_fpoint_kernel(long long G, int xid, int cid, double dfx, double dfc, double x_alpha, double *__restrict__ rho,
                                 const double *__restrict__ w, double *__restrict__ uS, double *__restrict__ uT, double *__restrict__ fpts)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const double n = fmax(rho[g], 1e-23);
    double fX = 0.0, fS = 0.0, fT = 0.0;
    if (xid == X_SLATER) fX = 2.0 * slater_d2f(n, x_alpha);
    if (cid == C_VWN5 || cid == C_VWN3) {
        double d2f, fmm;
        if (cid == C_VWN5) vwn5_kernel(n, d2f, fmm); else vwn3_kernel(n, d2f, fmm);
        fS = 2.0 * d2f; fT = 2.0 * fmm;
    }
    rho[g] = n;
    uS[g] = w[g] * (dfx * fX + dfc * fS);
    uT[g] = w[g] * (dfx * fX + dfc * fT);
    if (fpts) { fpts[g] = n; fpts[G + g] = fX; fpts[2 * G + g] = fS; fpts[3 * G + g] = fT; }
}

// D[g][n] = w (vrho phi + 4 vsig sum_a grad_a dphi_a)
__global__ void xc_dmat_kernel(long long G, int N, const double *__restrict__ w, const double *__restrict__ phi,
                               const double *__restrict__ dphi, const double *__restrict__ grad, const double *__restrict__ vrho,
                               const double *__restrict__ vsig, int gga, double *__restrict__ D)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * N) return;
    const long long g = e / N;
    double v = vrho[g] * phi[e];
    if (gga) v += 4.0 * vsig[g] * (grad[g] * dphi[e] + grad[G + g] * dphi[G * N + e] + grad[2 * G + g] * dphi[2 * G * N + e]);
    D[e] = w[g] * v;
}

// partial sums of w*rho, w*ex, w*ec
__global__ void xc_reduce_kernel(long long G, const double *__restrict__ w, const double *__restrict__ rho, const double *__restrict__ ex,
                                 const double *__restrict__ ec, double *__restrict__ part)
{
    __shared__ double s0[256], s1[256], s2[256];
    double a = 0, b = 0, c = 0;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (long long)gridDim.x * blockDim.x) {
        a += w[g] * rho[g]; b += w[g] * ex[g]; c += w[g] * ec[g];
    }
    s0[threadIdx.x] = a; s1[threadIdx.x] = b; s2[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) { s0[threadIdx.x] += s0[threadIdx.x + s]; s1[threadIdx.x] += s1[threadIdx.x + s]; s2[threadIdx.x] += s2[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = s0[0]; part[3 * blockIdx.x + 1] = s1[0]; part[3 * blockIdx.x + 2] = s2[0]; }
}

// tmp = sum_s in[s] over the nparts split-K partials (fixed order; coalesced), then out = sym(tmp)
__global__ void sum_parts_kernel(const double *__restrict__ in, int nparts, double *__restrict__ tmp, int nn)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nn) return;
    double a = 0.0;
    for (int s = 0; s < nparts; ++s) a += in[(size_t)s * nn + e];
    tmp[e] = a;
}
__global__ void sym_kernel(const double *__restrict__ tmp, double *__restrict__ out, int n)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int i = e / n, j = e - i * n;
    out[e] = (1.0 / 2.0) * (tmp[e] + tmp[(size_t)j * n + i]);
}

// ---- unrestricted (spin-polarised) path: calculate_unrestricted_exchange_correlation_matrix, tuna_scf.py:665-750 --------------------
// Exchange of spin s is the closed-shell functional at (2 rho_s, 4 sigma_ss), integrated against rho_s (tuna_scf.py:467-468, :719-741);
// correlation is the spin-polarised functional of (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb).  Per point and spin the D row is
//     D_s = w (v_rho_s Phi + c_s . grad Phi),   c_s = 4 (2 DFX dfds_X,s + DFC v_sigma_ss) grad rho_s + 2 DFC v_sigma_ab grad rho_s'
// (calculate_V_X / calculate_V_C, tuna_dft.py:788-888).  Both spins share every pass over Phi and grad Phi: the density kernel reads
// them once for both B rows, the D kernel reads them once and writes both D rows; the two GEMMs run on 2N-wide operands.
// Floors as the reference: rho_s >= 1e-23 each, sigma_ss >= 1e-46, sigma_ab not floored, zeta clipped to [-1, 1] (tuna_dft.py:677-744,
// tuna_xc.py:31-125).

struct XcSpin { double va, vb, vaa, vbb, vab, e; };            // df/drho_a, df/drho_b, df/dsigma_aa, _bb, _ab; energy per particle

__device__ inline void vwn_pot(double n, double x_0, double b, double c, double A, double &e, double &dedr)   // tuna_xc.py:1802-1860
{
    const double Q = sqrt(4.0 * c - b * b);
    const double X_0 = x_0 * x_0 + b * x_0 + c;
    const double c_1 = -b * x_0 / X_0;
    const double c_2 = 2.0 * b * (c - x_0 * x_0) / (Q * X_0);
    const double r_s = cbrt(3.0 / (4.0 * 3.141592653589793) * (1.0 / n));
    const double x = sqrt(r_s);
    const double xm = x - x_0;
    const double Xx = r_s + b * x + c;
    const double combo = (2.0 / x + 2.0 * c_1 / xm - (2.0 * x + b) * (1.0 + c_1) / Xx - (1.0 / 2.0) * c_2 * Q / Xx);
    e = A * (log(r_s / Xx) + c_1 * log(xm * xm / Xx) + c_2 * atan(Q / (2.0 * x + b)));
    dedr = (A / 2.0) * combo / x;
}

__device__ inline double spin_f(double z)                       // tuna_xc.py:126-178
{
    const double p = cbrt(1.0 + z), m = cbrt(1.0 - z), t = cbrt(2.0);
    return (p * p * p * p + m * m * m * m - 2.0) / (t * t * t * t - 2.0);
}
__device__ inline double spin_fp(double z)
{
    const double t = cbrt(2.0);
    return (cbrt(1.0 + z) - cbrt(1.0 - z)) / (t * t * t * t - 2.0) * 4.0 / 3.0;
}

__device__ inline XcSpin vwn3_spin(double na, double nb, double n)                 // tuna_xc.py:1542-1600
{
    double e0, d0, e1, d1;
    vwn_pot(n, -0.409286, 13.0720, 42.7198, 0.0310907, e0, d0);
    vwn_pot(n, -0.743294, 20.1231, 101.578, 0.01554535, e1, d1);
    const double z = fmin(fmax((na - nb) / (na + nb), -1.0), 1.0);
    const double f = spin_f(z), fp = spin_fp(z);
    const double r_s = cbrt(3.0 / (4.0 * 3.141592653589793) * (1.0 / n));
    XcSpin o{0, 0, 0, 0, 0, 0};
    o.e = e0 + (e1 - e0) * f;
    const double dedr = d0 + (d1 - d0) * f, dedz = (e1 - e0) * fp;
    o.va = o.e - r_s / 3.0 * dedr - (z - 1.0) * dedz;
    o.vb = o.e - r_s / 3.0 * dedr - (z + 1.0) * dedz;
    return o;
}

__device__ inline XcSpin vwn5_spin(double na, double nb, double n)                 // tuna_xc.py:1631-1669, :1870-1935
{
    double e0, d0, e1, d1, ma, dma;
    vwn_pot(n, -0.10498, 3.72744, 12.9352, 0.0310907, e0, d0);
    vwn_pot(n, -0.32500, 7.06042, 18.0578, 0.01554535, e1, d1);
    vwn_pot(n, -0.0047584, 1.13107, 13.0045, 1.0 / (6.0 * 3.141592653589793 * 3.141592653589793), ma, dma);
    const double alpha = -ma, dalpha_dr = -dma;
    const double z = fmin(fmax((na - nb) / (na + nb), -1.0), 1.0);
    const double z4 = z * z * z * z;
    const double f = spin_f(z), fp = spin_fp(z);
    const double t = cbrt(2.0), fpp0 = 8.0 / (9.0 * (t * t * t * t - 2.0));
    XcSpin o{0, 0, 0, 0, 0, 0};
    o.e = e0 + alpha * f / fpp0 * (1.0 - z4) + (e1 - e0) * f * z4;
    const double r_s = cbrt(3.0 / (4.0 * 3.141592653589793) * (1.0 / n));
    const double dedr = d0 * (1.0 - f * z4) + d1 * f * z4 + dalpha_dr * f * (1.0 - z4) / fpp0;
    const double dedz = 4.0 * z * z * z * f * (e1 - e0 - alpha / fpp0) + fp * (z4 * (e1 - e0) + (1.0 - z4) * alpha / fpp0);
    o.va = o.e - r_s / 3.0 * dedr - (z - 1.0) * dedz;
    o.vb = o.e - r_s / 3.0 * dedr - (z + 1.0) * dedz;
    return o;
}

__device__ inline XcSpin lyp_spin(double na, double nb, double n, double saa, double sbb, double sab)   // tuna_xc.py:2271-2370
{
    const double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
    const double PI = 3.141592653589793;
    const double ca = cbrt(na), cb = cbrt(nb);
    const double inv_n = 1.0 / n;
    const double cn = cbrt(n), icn = 1.0 / cn;
    const double X = 1.0 + d * icn;
    const double t = cbrt(2.0), k = cbrt(3.0 * PI * PI);
    const double t2 = t * t, t4 = t2 * t2, t8 = t4 * t4;
    const double C = t8 * t2 * t * 3.0 / 10.0 * (k * k);
    const double prod = na * nb;
    const double ca2 = ca * ca, ca4 = ca2 * ca2, ca8 = ca4 * ca4, cb2 = cb * cb, cb4 = cb2 * cb2, cb8 = cb4 * cb4;
    const double psum = ca8 + cb8;
    const double icn2 = icn * icn, icn4 = icn2 * icn2, icn8 = icn4 * icn4;
    const double w = icn8 * icn2 * icn * exp(-c * icn) / X;
    const double delta = icn * (c + d / X);
    const double mabw = -a * b * w;
    const double w_prime = -(1.0 / 3.0) * icn4 * w * (11.0 * cn - c - d / X);
    const double delta_prime = (1.0 / 3.0) * (d * d * icn4 * icn / (X * X) - delta * inv_n);
    const double wpw = -(1.0 / 3.0) * icn4 * (11.0 * cn - c - d / X);
    XcSpin o;
    o.vaa = mabw * ((1.0 / 9.0) * prod * (1.0 - 3.0 * delta - (delta - 11.0) * na * inv_n) - nb * nb);
    o.vbb = mabw * ((1.0 / 9.0) * prod * (1.0 - 3.0 * delta - (delta - 11.0) * nb * inv_n) - na * na);
    o.vab = mabw * ((1.0 / 9.0) * prod * (47.0 - 7.0 * delta) - (4.0 / 3.0) * n * n);
    o.e = inv_n * (prod * (C * mabw * psum - 4.0 * a / X * inv_n) + o.vaa * saa + o.vbb * sbb + o.vab * sab);
    const double d_a_aa = wpw * o.vaa + mabw * ((1.0 / 9.0) * nb * (1.0 - 3.0 * delta - (delta - 11.0) * na * inv_n) -
                                                (1.0 / 9.0) * prod * (delta_prime * (3.0 + na * inv_n) + (delta - 11.0) * nb * inv_n * inv_n));
    const double d_b_bb = wpw * o.vbb + mabw * ((1.0 / 9.0) * na * (1.0 - 3.0 * delta - (delta - 11.0) * nb * inv_n) -
                                                (1.0 / 9.0) * prod * (delta_prime * (3.0 + nb * inv_n) + (delta - 11.0) * na * inv_n * inv_n));
    const double d_a_ab = wpw * o.vab + mabw * ((1.0 / 9.0) * nb * (47.0 - 7.0 * delta) - (7.0 / 9.0) * prod * delta_prime - (8.0 / 3.0) * n);
    const double d_b_ab = wpw * o.vab + mabw * ((1.0 / 9.0) * na * (47.0 - 7.0 * delta) - (7.0 / 9.0) * prod * delta_prime - (8.0 / 3.0) * n);
    const double d_a_bb = wpw * o.vbb + mabw * ((1.0 / 9.0) * nb * (1.0 - 3.0 * delta - (delta - 11.0) * nb * inv_n) -
                                                (1.0 / 9.0) * prod * ((3.0 + nb * inv_n) * delta_prime - (delta - 11.0) * nb * inv_n * inv_n) - 2.0 * na);
    const double d_b_aa = wpw * o.vaa + mabw * ((1.0 / 9.0) * na * (1.0 - 3.0 * delta - (delta - 11.0) * na * inv_n) -
                                                (1.0 / 9.0) * prod * ((3.0 + na * inv_n) * delta_prime - (delta - 11.0) * na * inv_n * inv_n) - 2.0 * nb);
    o.va = -4.0 * a / X * prod * inv_n * ((1.0 / 3.0) * d * icn4 / X + 1.0 / na - inv_n) -
           C * a * b * (w_prime * prod * psum + w * nb * (11.0 / 3.0 * ca8 + cb8)) + d_a_aa * saa + d_a_bb * sbb + d_a_ab * sab;
    o.vb = -4.0 * a / X * prod * inv_n * ((1.0 / 3.0) * d * icn4 / X + 1.0 / nb - inv_n) -
           C * a * b * (w_prime * prod * psum + w * na * (11.0 / 3.0 * cb8 + ca8)) + d_b_bb * sbb + d_b_aa * saa + d_b_ab * sab;
    return o;
}

// (the rows of the spin set's per-point array pt [SPT][G]: tf_dft_plan.h)

// rho_s and grad rho_s of both spins from B2 = Phi [P_a | P_b]: sixteen lanes per grid point as xc_density_kernel, every Phi / grad Phi
// element read once for both spins
__global__ __launch_bounds__(256) void xc_density2_kernel(long long G, int N, const double *__restrict__ phi, const double *__restrict__ dphi,
                                                          const double *__restrict__ B2, int gga, double *__restrict__ pt)
{
    const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
    const long long g = (long long)blockIdx.x * 16 + grp;
    double na = 0.0, nb = 0.0, ax = 0.0, ay = 0.0, az = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
    if (g < G) {
        const double *ba = B2 + g * 2 * N, *bb = ba + N, *f = phi + g * N;
        if (gga) {
            const double *fx = dphi + g * N, *fy = dphi + G * N + g * N, *fz = dphi + 2 * G * N + g * N;
            for (int i = l; i < N; i += 16) {
                const double p = ba[i], q = bb[i], x = fx[i], y = fy[i], z = fz[i], v = f[i];
                na += p * v; nb += q * v;
                ax += p * x; ay += p * y; az += p * z;
                bx += q * x; by += q * y; bz += q * z;
            }
        } else {
            for (int i = l; i < N; i += 16) { const double v = f[i]; na += ba[i] * v; nb += bb[i] * v; }
        }
    }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) {
        na += __shfl_xor(na, d, 16); nb += __shfl_xor(nb, d, 16);
        ax += __shfl_xor(ax, d, 16); ay += __shfl_xor(ay, d, 16); az += __shfl_xor(az, d, 16);
        bx += __shfl_xor(bx, d, 16); by += __shfl_xor(by, d, 16); bz += __shfl_xor(bz, d, 16);
    }
    if (l == 0 && g < G) {
        pt[g] = na; pt[G + g] = nb;
        if (gga) {
            pt[2 * G + g] = 2.0 * ax; pt[3 * G + g] = 2.0 * ay; pt[4 * G + g] = 2.0 * az;
            pt[5 * G + g] = 2.0 * bx; pt[6 * G + g] = 2.0 * by; pt[7 * G + g] = 2.0 * bz;
        }
    }
}

__device__ inline XcOut exchange_of(int xid, double n, double sigma, double x_alpha)
{
    XcOut X{0, 0, 0};
    if (xid == X_SLATER) X = slater_x(n, x_alpha);
    else if (xid == X_B88) X = b88_x(n, sigma, x_alpha);
    else if (xid == X_B3) {                                                 // 0.9 B88 + 0.1 Slater, tuna_xc.py:1462-1494
        const XcOut s = slater_x(n, x_alpha), bb = b88_x(n, sigma, x_alpha);
        X.dfdn = 0.9 * bb.dfdn + 0.1 * s.dfdn; X.dfds = 0.9 * bb.dfds; X.e = 0.9 * bb.e + 0.1 * s.e;
    }
    return X;
}

__device__ inline XcSpin correlation_of(int cid, double na, double nb, double n, double saa, double sbb, double sab)
{
    XcSpin C{0, 0, 0, 0, 0, 0};
    if (cid == C_VWN5) C = vwn5_spin(na, nb, n);
    else if (cid == C_VWN3) C = vwn3_spin(na, nb, n);
    else if (cid == C_LYP) C = lyp_spin(na, nb, n, saa, sbb, sab);
    else if (cid == C_3P_VWN5 || cid == C_3P_VWN3) {                        // 0.81 LYP + 0.19 VWN, tuna_xc.py:5893-5950
        const XcSpin l = (cid == C_3P_VWN5) ? vwn5_spin(na, nb, n) : vwn3_spin(na, nb, n);
        const XcSpin y = lyp_spin(na, nb, n, saa, sbb, sab);
        C.va = 0.81 * y.va + 0.19 * l.va; C.vb = 0.81 * y.vb + 0.19 * l.vb;
        C.vaa = 0.81 * y.vaa; C.vbb = 0.81 * y.vbb; C.vab = 0.81 * y.vab;
        C.e = 0.81 * y.e + 0.19 * l.e;
    }
    return C;
}

__global__ void xc_point2_kernel(long long G, int gga, int xid, int cid, double dfx, double dfc, double x_alpha, double *__restrict__ pt)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const double na = fmax(pt[g], 1e-23), nb = fmax(pt[G + g], 1e-23);
    const double n = na + nb;
    double ga[3] = {0.0, 0.0, 0.0}, gb[3] = {0.0, 0.0, 0.0};
    if (gga)
        for (int a = 0; a < 3; ++a) { ga[a] = pt[(2 + a) * G + g]; gb[a] = pt[(5 + a) * G + g]; }
    const double saa = fmax(ga[0] * ga[0] + ga[1] * ga[1] + ga[2] * ga[2], 1e-46);
    const double sbb = fmax(gb[0] * gb[0] + gb[1] * gb[1] + gb[2] * gb[2], 1e-46);
    const double sab = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
    const XcOut Xa = exchange_of(xid, 2.0 * na, 4.0 * saa, x_alpha), Xb = exchange_of(xid, 2.0 * nb, 4.0 * sbb, x_alpha);
    const XcSpin C = correlation_of(cid, na, nb, n, saa, sbb, sab);
    pt[g] = na; pt[G + g] = nb;
    pt[8 * G + g] = dfx * Xa.dfdn + dfc * C.va;
    pt[9 * G + g] = dfx * Xb.dfdn + dfc * C.vb;
    if (gga) {
        const double ka = 4.0 * (dfx * 2.0 * Xa.dfds + dfc * C.vaa), kb = 4.0 * (dfx * 2.0 * Xb.dfds + dfc * C.vbb), kab = 2.0 * dfc * C.vab;
        for (int a = 0; a < 3; ++a) {
            pt[(10 + a) * G + g] = ka * ga[a] + kab * gb[a];
            pt[(13 + a) * G + g] = kb * gb[a] + kab * ga[a];
        }
    }
    pt[16 * G + g] = Xa.e * na;
    pt[17 * G + g] = Xb.e * nb;
    pt[18 * G + g] = C.e * n;
}

// ---- spin-resolved second derivatives of the local-density functionals: the exchange-correlation kernel of unrestricted TD-DFT and of
// the Kohn-Sham stability analysis (calculate_unrestricted_exchange_correlation_kernel_matrices, tuna_dft.py:1233-1248) -----------------
//     f_X,ss = 2 f_X(2 rho_s) with the bare Slater function (slater_d2f, not the restricted kernel's doubled f_X); f_X,ab = 0
//     f_C,st = d2(n e_C)/d rho_s d rho_t in the variables (n, zeta) through the chain rule (VWN3: tuna_xc.py:6072-6140; VWN5: :6308-6438)
// Guards as the reference: rho_s floored at 1e-23 each (the caller), zeta clipped to [-1, 1], 1 +- zeta floored at 1e-23 in f''(zeta) only.

struct XcSpinKernel { double faa, fab, fbb; };

// The chain rule from (n, zeta) to (rho_a, rho_b), in one fixed order of its terms: faa(rho_a, rho_b) and fbb(rho_b, rho_a) are the same
// operations on the same numbers wherever the call is inlined
__device__ __forceinline__ XcSpinKernel spin_chain(double n, double z, double r_s, double de_dr, double d2e_dr2, double de_dz, double d2e_dz2,
                                                   double d2e_drdz)
{
#pragma clang fp contract(off)
    const double f_nn = (r_s * r_s * d2e_dr2 - 2.0 * r_s * de_dr) / (9.0 * n);
    const double f_nz = de_dz - (r_s / 3.0) * d2e_drdz;
    const double f_zz = n * d2e_dz2;
    const double f_z = n * de_dz;
    const double n2 = n * n;
    const double zu = (1.0 - z) / n, zw = -(1.0 + z) / n;
    const double zuu = -2.0 * (1.0 - z) / n2, zww = 2.0 * (1.0 + z) / n2, zuw = 2.0 * z / n2;
    XcSpinKernel o;
    o.faa = ((f_nn + 2.0 * f_nz * zu) + f_zz * (zu * zu)) + f_z * zuu;
    o.fbb = ((f_nn + 2.0 * f_nz * zw) + f_zz * (zw * zw)) + f_z * zww;
    o.fab = ((f_nn + f_nz * (zu + zw)) + f_zz * (zu * zw)) + f_z * zuw;
    return o;
}

// f''(zeta) of the spin-scaling function with the reference's floor at full polarisation
__device__ inline double spin_fpp(double z)
{
    const double t = cbrt(2.0);
    const double p = cbrt(fmax(1.0 + z, 1e-23)), m = cbrt(fmax(1.0 - z, 1e-23));
    return (4.0 / 9.0) * (1.0 / (p * p) + 1.0 / (m * m)) / (t * t * t * t - 2.0);
}

__device__ inline XcSpinKernel vwn3_spin_kernel(double na, double nb, double n)       // tuna_xc.py:6072-6140
{
    const VwnD2 p0 = vwn_d2(n, -0.409286, 13.0720, 42.7198, 0.0310907), p1 = vwn_d2(n, -0.743294, 20.1231, 101.578, 0.01554535);
    const double z = fmin(fmax((na - nb) / (na + nb), -1.0), 1.0);
    const double f = spin_f(z), fp = spin_fp(z), fpp = spin_fpp(z);
    const double de_dr = p0.dedr * (1.0 - f) + p1.dedr * f;
    const double d2e_dr2 = p0.d2edr2 * (1.0 - f) + p1.d2edr2 * f;
    const double de_dz = (p1.e - p0.e) * fp, d2e_dz2 = (p1.e - p0.e) * fpp, d2e_drdz = (p1.dedr - p0.dedr) * fp;
    return spin_chain(n, z, p0.r_s, de_dr, d2e_dr2, de_dz, d2e_dz2, d2e_drdz);
}

__device__ inline XcSpinKernel vwn5_spin_kernel(double na, double nb, double n)       // tuna_xc.py:6308-6438
{
    const VwnD2 p0 = vwn_d2(n, -0.10498, 3.72744, 12.9352, 0.0310907), p1 = vwn_d2(n, -0.32500, 7.06042, 18.0578, 0.01554535),
                pa = vwn_d2(n, -0.0047584, 1.13107, 13.0045, 1.0 / (6.0 * 3.141592653589793 * 3.141592653589793));
    const double al = -pa.e, dal = -pa.dedr, d2al = -pa.d2edr2;                     // the spin stiffness and its r_s derivatives
    const double z = fmin(fmax((na - nb) / (na + nb), -1.0), 1.0);
    const double t = cbrt(2.0), fpp0 = 8.0 / (9.0 * (t * t * t * t - 2.0));
    const double f = spin_f(z), fp = spin_fp(z), fpp = spin_fpp(z);
    const double z2 = z * z, z3 = z2 * z, z4 = z3 * z;
    const double h = f * z4, hp = fp * z4 + 4.0 * f * z3, hpp = fpp * z4 + 8.0 * fp * z3 + 12.0 * f * z2;
    const double g = f * (1.0 - z4) / fpp0, gp = (fp * (1.0 - z4) - 4.0 * f * z3) / fpp0,
                 gpp = (fpp * (1.0 - z4) - 8.0 * fp * z3 - 12.0 * f * z2) / fpp0;
    const double de_dr = p0.dedr * (1.0 - h) + p1.dedr * h + dal * g;
    const double d2e_dr2 = p0.d2edr2 * (1.0 - h) + p1.d2edr2 * h + d2al * g;
    const double de_dz = (p1.e - p0.e) * hp + al * gp, d2e_dz2 = (p1.e - p0.e) * hpp + al * gpp;
    const double d2e_drdz = (p1.dedr - p0.dedr) * hp + dal * gp;
    return spin_chain(n, z, p0.r_s, de_dr, d2e_dr2, de_dz, d2e_dz2, d2e_drdz);
}

// rho_a, rho_b (rows 0, 1 of pt: xc_density2_kernel's sums, floored here as in xc_point2_kernel) of a point; the three weights of the
// spin-blocked kernel matrix  u[0] = u_aa = w (dfx f_X,aa + dfc f_C,aa),  u[1] = u_ab = w dfc f_C,ab,  u[2] = u_bb likewise  ([3][G]);
// fpts (may be null): [7][G] = rho_a, rho_b, f_X,aa, f_X,bb, f_C,aa, f_C,ab, f_C,bb.  Local-density ids only (the caller refuses the others).
__global__ void xc_fpoint2_kernel(long long G, int xid, int cid, double dfx, double dfc, double x_alpha, double *__restrict__ pt,
                                  const double *__restrict__ w, double *__restrict__ u, double *__restrict__ fpts)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const double na = fmax(pt[g], 1e-23), nb = fmax(pt[G + g], 1e-23);
    const double n = na + nb;
    double fXa = 0.0, fXb = 0.0;
    XcSpinKernel C{0.0, 0.0, 0.0};
    if (xid == X_SLATER) { fXa = 2.0 * slater_d2f(2.0 * na, x_alpha); fXb = 2.0 * slater_d2f(2.0 * nb, x_alpha); }
    if (cid == C_VWN5) C = vwn5_spin_kernel(na, nb, n);
    else if (cid == C_VWN3) C = vwn3_spin_kernel(na, nb, n);
    pt[g] = na; pt[G + g] = nb;
    u[g] = w[g] * (dfx * fXa + dfc * C.faa);
    u[G + g] = w[g] * (dfc * C.fab);
    u[2 * G + g] = w[g] * (dfx * fXb + dfc * C.fbb);
    if (fpts) {
        fpts[g] = na; fpts[G + g] = nb; fpts[2 * G + g] = fXa; fpts[3 * G + g] = fXb;
        fpts[4 * G + g] = C.faa; fpts[5 * G + g] = C.fab; fpts[6 * G + g] = C.fbb;
    }
}

// D2[g][s N + i] = w (v_rho_s phi + c_s . grad phi): one element of Phi (and of grad Phi) per thread, both spins written
__global__ void xc_dmat2_kernel(long long G, int N, const double *__restrict__ w, const double *__restrict__ phi, const double *__restrict__ dphi,
                                const double *__restrict__ pt, int gga, double *__restrict__ D2)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * N) return;
    const long long g = e / N;
    const long long i = e - g * N;
    const double f = phi[e];
    double va = pt[8 * G + g] * f, vb = pt[9 * G + g] * f;
    if (gga) {
        const double x = dphi[e], y = dphi[G * N + e], z = dphi[2 * G * N + e];
        va += pt[10 * G + g] * x + pt[11 * G + g] * y + pt[12 * G + g] * z;
        vb += pt[13 * G + g] * x + pt[14 * G + g] * y + pt[15 * G + g] * z;
    }
    const double wg = w[g];
    D2[g * 2 * N + i] = wg * va;
    D2[g * 2 * N + N + i] = wg * vb;
}

// partial sums of w rho_a, w rho_b, w e_X,a rho_a, w e_X,b rho_b, w e_C rho
__global__ __launch_bounds__(256) void xc_reduce5_kernel(long long G, const double *__restrict__ w, const double *__restrict__ pt,
                                                         double *__restrict__ part)
{
    __shared__ double sm[5][256];
    const int rows[5] = {0, 1, 16, 17, 18};
    double acc[5] = {0, 0, 0, 0, 0};
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (long long)gridDim.x * blockDim.x) {
        const double wg = w[g];
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q] += wg * pt[rows[q] * G + g];
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) sm[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int q = 0; q < 5; ++q) sm[q][threadIdx.x] += sm[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 5) part[5 * blockIdx.x + threadIdx.x] = sm[threadIdx.x][0];
}

// P2[k][s N + i] = P_s[k][i]: the two densities as one N x 2N operand
__global__ void pack2_kernel(const double *__restrict__ Pa, const double *__restrict__ Pb, double *__restrict__ P2, int N)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2LL * N * N) return;
    const long long k = e / (2 * N);
    const long long r = e - k * 2 * N;
    P2[e] = r < N ? Pa[k * N + r] : Pb[k * N + (r - N)];
}

// out_s = sym(V_s) from the summed [N][2N] product (row j holds (Phi^T D_s)[:, j] of both spins)
__global__ void sym2_kernel(const double *__restrict__ tmp, double *__restrict__ Va, double *__restrict__ Vb, int N)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nn = (long long)N * N;
    if (e >= 2 * nn) return;
    const int s = (int)(e / nn);
    const long long q = e - s * nn;
    const long long r = q / N, c = q - r * N;
    (s ? Vb : Va)[q] = (1.0 / 2.0) * (tmp[r * 2 * N + s * N + c] + tmp[c * 2 * N + s * N + r]);
}

}  // namespace tfdft
