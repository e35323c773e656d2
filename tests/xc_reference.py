"""TEST INFRASTRUCTURE ONLY -- an independent CPU reference of tf_dft_vxc (tuna_amd/csrc/tf_dft.hip.h), written from the math.

It imports none of the library's DFT code.  What it computes:
  * contracted Cartesian Gaussians and their gradients on grid points, normalised in closed form (primitive norm, then contraction
    renormalisation), optionally mapped to the real spherical harmonics by tuna_amd.spherical.transformation_matrix;
  * rho = sum P_ij phi_i phi_j, grad rho = 2 sum P_ij phi_i grad phi_j (this operand order matters for a non-symmetric P),
    sigma = |grad rho|^2, floored as the kernel floors them (rho at 1e-23, sigma at 1e-46);
  * the functionals as energy densities f(n, sigma) = n e(n, sigma) ONLY: Slater (tuna_xc.py:199-213), B88 (:385-438), B3 (:1462-1494),
    VWN5 / VWN3 (:1512-1630, :1802-1860), LYP (:2200-2260), 3P and 3P/G (:5843-5881), with the constants of tf_dft.hip.h.
    v_rho = df/dn and v_sigma = df/dsigma come from complex-step differentiation (NumPy, every function involved is analytic on the
    positive axis) or from mpmath's numerical derivative at 40 digits for single points -- never from hand-derived formulas;
  * V = sym(Phi^T W (v_rho Phi + 4 v_sigma grad rho . grad Phi)), n_el = sum w rho, E_X = dfx sum w f_x, E_C = dfc sum w f_c.
"""
from __future__ import annotations

from math import pi as PI

import numpy as np

X_NONE, X_SLATER, X_B88, X_B3 = 0, 1, 2, 3
C_NONE, C_VWN5, C_VWN3, C_LYP, C_3P_VWN5, C_3P_VWN3 = 0, 1, 2, 3, 4, 5
RHO_FLOOR, SIGMA_FLOOR = 1e-23, 1e-46
VWN5 = (-0.10498, 3.72744, 12.9352, 0.0310907)           # (x_0, b, c, A), paramagnetic
VWN3 = (-0.409286, 13.0720, 42.7198, 0.0310907)


# ---- math back ends: NumPy (real or complex arrays) and mpmath ---------------------------------------------------------------

class _NP:
    sqrt, log, exp, atan, asinh = np.sqrt, np.log, np.exp, np.arctan, np.arcsinh
    pi = PI

    @staticmethod
    def cbrt(x):
        return x ** (1.0 / 3.0)                            # principal branch; np.cbrt has no complex form


class _MP:
    def __init__(self):
        import mpmath
        self.m = mpmath
        self.sqrt, self.log, self.exp, self.atan, self.asinh = mpmath.sqrt, mpmath.log, mpmath.exp, mpmath.atan, mpmath.asinh

    @property
    def pi(self):
        return self.m.pi

    def cbrt(self, x):
        return self.m.cbrt(x)


# ---- energy densities f = n e(n, sigma) ------------------------------------------------------------------------------------------

def slater(M, n, x_alpha):
    """Slater-Dirac exchange with the X-alpha scaling: e = -(9/8) alpha (3 n / pi)^(1/3)."""
    return n * (-(9.0 / 8.0) * x_alpha * M.cbrt(3.0 * n / M.pi))


def b88(M, n, sigma, x_alpha):
    """Becke 88 for the closed shell: two spin channels of density n/2 and gradient sigma/4; per channel
    e_sigma = C e_LDA(n_s) - beta n_s^(1/3) x^2 / (1 + 6 beta x asinh x), x = |grad n_s| / n_s^(4/3), C = 2 / 4^(1/3)."""
    beta = 0.0042
    ns = n / 2.0
    e_lda = -(9.0 / 8.0) * x_alpha * M.cbrt(3.0 * ns / M.pi)
    c3 = M.cbrt(ns)
    x = M.sqrt(sigma / 4.0) / (c3 * c3 * c3 * c3)
    e = (2.0 / M.cbrt(4.0)) * e_lda - beta * c3 * x * x / (1.0 + 6.0 * beta * x * M.asinh(x))
    return n * e


def vwn(M, n, params):
    """Vosko-Wilk-Nusair paramagnetic correlation: e = A [ln(x^2/X) + c1 ln((x - x0)^2 / X) + c2 atan(Q / (2x + b))],
    x = sqrt(r_s), X(x) = x^2 + b x + c, Q = sqrt(4c - b^2), c1 = -b x0 / X(x0), c2 = 2 b (c - x0^2) / (Q X(x0))."""
    x0, b, c, A = params
    Q = (4.0 * c - b * b) ** 0.5
    X0 = x0 * x0 + b * x0 + c
    c1 = -b * x0 / X0
    c2 = 2.0 * b * (c - x0 * x0) / (Q * X0)
    rs = M.cbrt(3.0 / (4.0 * M.pi * n))
    x = M.sqrt(rs)
    Xx = rs + b * x + c
    e = A * (M.log(rs / Xx) + c1 * M.log((x - x0) * (x - x0) / Xx) + c2 * M.atan(Q / (2.0 * x + b)))
    return n * e


def lyp(M, n, sigma):
    """Lee-Yang-Parr for the closed shell in the Miehlich form:
    e = -a / X - a b w n [C_F' n^(8/3) / 2 ... ] with X = 1 + d n^(-1/3), w = n^(-11/3) exp(-c n^(-1/3)) / X,
    delta = n^(-1/3) (c + d / X), C2 = (3/10)(3 pi^2)^(2/3) 2 n^(8/3):
    e = (1/2) C2 (-a b w n) - (-a b w n) sigma (7 delta + 3) / 72 - a / X."""
    a, b, c, d = 0.04918, 0.132, 0.2533, 0.349
    c3 = M.cbrt(n)
    ic3 = 1.0 / c3
    X = 1.0 + d * ic3
    k = M.cbrt(3.0 * M.pi * M.pi)
    C2 = 6.0 / 10.0 * k * k * c3 ** 8
    w = ic3 ** 11 * M.exp(-c * ic3) / X
    delta = ic3 * (c + d / X)
    mabw = -a * b * w * n
    e = 0.5 * C2 * mabw - mabw * sigma * (7.0 * delta + 3.0) / 72.0 - a / X
    return n * e


def f_x(M, xid, n, sigma, x_alpha):
    if xid == X_SLATER:
        return slater(M, n, x_alpha)
    if xid == X_B88:
        return b88(M, n, sigma, x_alpha)
    if xid == X_B3:
        return 0.9 * b88(M, n, sigma, x_alpha) + 0.1 * slater(M, n, x_alpha)
    return 0.0 * n


def f_c(M, cid, n, sigma):
    if cid == C_VWN5:
        return vwn(M, n, VWN5)
    if cid == C_VWN3:
        return vwn(M, n, VWN3)
    if cid == C_LYP:
        return lyp(M, n, sigma)
    if cid in (C_3P_VWN5, C_3P_VWN3):
        return 0.81 * lyp(M, n, sigma) + 0.19 * vwn(M, n, VWN5 if cid == C_3P_VWN5 else VWN3)
    return 0.0 * n


def floors(rho, sigma):
    return np.maximum(rho, RHO_FLOOR), np.maximum(sigma, SIGMA_FLOOR)


def complex_step(fn, n, sigma):
    """(f, df/dn, df/dsigma) of fn(M, n, sigma) at floored, positive n and sigma, by complex steps h = 1e-30 x."""
    n = np.asarray(n, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    hn, hs = 1e-30 * n, 1e-30 * sigma
    f = fn(_NP, n, sigma)
    dn = np.imag(fn(_NP, n + 1j * hn, sigma.astype(complex))) / hn
    ds = np.imag(fn(_NP, n.astype(complex), sigma + 1j * hs)) / hs
    return np.real(f) * np.ones_like(n), dn * np.ones_like(n), ds * np.ones_like(n)


def point_derivs(xid, cid, n, sigma, x_alpha=2.0 / 3.0):
    """Complex-step (f_x, f_c, dfx/dn, dfx/ds, dfc/dn, dfc/ds) on arrays of floored points."""
    fx, xn, xs = complex_step(lambda M, a, s: f_x(M, xid, a, s, x_alpha), n, sigma)
    fc, cn, cs = complex_step(lambda M, a, s: f_c(M, cid, a, s), n, sigma)
    return fx, fc, xn, xs, cn, cs


def mp_point(xid, cid, n, sigma, x_alpha=2.0 / 3.0, dps=40):
    """The same six numbers for ONE floored point with mpmath at `dps` digits (mp.diff), as floats."""
    import mpmath
    M = _MP()
    with mpmath.workdps(dps + 20):
        n_, s_, xa = mpmath.mpf(float(n)), mpmath.mpf(float(sigma)), mpmath.mpf(float(x_alpha))
        hn, hs = n_ * mpmath.mpf(10) ** -15, s_ * mpmath.mpf(10) ** -15           # relative central-difference steps
        fx = lambda a, s: f_x(M, xid, a, s, xa) if xid else mpmath.mpf(0)   # noqa: E731
        fc = lambda a, s: f_c(M, cid, a, s) if cid else mpmath.mpf(0)        # noqa: E731
        out = [fx(n_, s_), fc(n_, s_),
               mpmath.diff(lambda a: fx(a, s_), n_, h=hn), mpmath.diff(lambda s: fx(n_, s), s_, h=hs),
               mpmath.diff(lambda a: fc(a, s_), n_, h=hn), mpmath.diff(lambda s: fc(n_, s), s_, h=hs)]
        return tuple(float(v) for v in out)


# ---- AOs on points -----------------------------------------------------------------------------------------------------------

def _dfact(k):
    r = 1.0
    while k > 1:
        r *= k
        k -= 2
    return r


def ao_weights(aos):
    """Per-primitive weight N_p c_p N_contr of every Cartesian AO: the primitive norm
    N_p = (2 a / pi)^(3/4) (4 a)^(L/2) / sqrt((2l-1)!! (2m-1)!! (2n-1)!!), then the contracted AO is scaled to unit self-overlap
    using <g_p|g_q> = (pi / (a_p + a_q))^(3/2) (2l-1)!! (2m-1)!! (2n-1)!! / (2 (a_p + a_q))^L."""
    w = np.empty_like(aos.exps)
    for i in range(aos.n):
        lo, hi = int(aos.prim_off[i]), int(aos.prim_off[i + 1])
        l, m, n = (int(v) for v in aos.lmn[i])
        L = l + m + n
        a, c = aos.exps[lo:hi], aos.coefs[lo:hi]
        df = _dfact(2 * l - 1) * _dfact(2 * m - 1) * _dfact(2 * n - 1)
        Np = (2.0 * a / PI) ** 0.75 * (4.0 * a) ** (L / 2.0) / np.sqrt(df)
        ab = a[:, None] + a[None, :]
        S = (PI / ab) ** 1.5 * df / (2.0 * ab) ** L
        cn = c * Np
        w[lo:hi] = cn / np.sqrt(cn @ S @ cn)
    return w


def ao_on_points(aos, pts, U=None, weights=None, with_grad=True):
    """phi [G, N] and grad phi [3, G, N] (None without with_grad) at points [3, G] (Cartesian AOs, or spherical ones if
    U [n_sph, n_cart] is given)."""
    w = ao_weights(aos) if weights is None else weights
    X, Y, Z = (np.asarray(p, dtype=np.float64) for p in pts)
    G, n = X.size, aos.n
    phi, dphi = np.empty((G, n)), (np.empty((3, G, n)) if with_grad else None)
    cache = {}
    for i in range(n):
        lo, hi = int(aos.prim_off[i]), int(aos.prim_off[i + 1])
        z0 = float(aos.origin[i, 2])
        assert aos.origin[i, 0] == 0.0 and aos.origin[i, 1] == 0.0
        zr = Z - z0
        key = (z0, tuple(aos.exps[lo:hi]))
        if key not in cache:
            r2 = X * X + Y * Y + zr * zr
            cache[key] = np.exp(-np.outer(aos.exps[lo:hi], r2))          # [nprim, G]
        E = cache[key]
        s = w[lo:hi] @ E                                                  # sum_p w_p e^{-a r^2}
        l, m, k = (int(v) for v in aos.lmn[i])
        px, py, pz = X ** l, Y ** m, zr ** k
        poly = px * py * pz
        phi[:, i] = poly * s
        if not with_grad:
            continue
        sa = (w[lo:hi] * aos.exps[lo:hi]) @ E                             # sum_p w_p a_p e^{-a r^2}
        dx = (l * X ** (l - 1) * py * pz if l else 0.0)
        dy = (m * Y ** (m - 1) * px * pz if m else 0.0)
        dz = (k * zr ** (k - 1) * px * py if k else 0.0)
        dphi[0, :, i] = dx * s - 2.0 * X * poly * sa
        dphi[1, :, i] = dy * s - 2.0 * Y * poly * sa
        dphi[2, :, i] = dz * s - 2.0 * zr * poly * sa
    if U is not None:
        phi = phi @ U.T
        dphi = dphi @ U.T if with_grad else None
    return phi, dphi


def overlap_on_grid(aos, pts, wts, U=None, chunk=20000):
    """sum_g w_g phi_i(g) phi_j(g): the quadrature of the overlap matrix."""
    pts = np.asarray(pts).reshape(3, -1)
    wts = np.asarray(wts).reshape(-1)
    w = ao_weights(aos)
    N = aos.n if U is None else U.shape[0]
    S = np.zeros((N, N))
    for a in range(0, wts.size, chunk):
        phi, _ = ao_on_points(aos, pts[:, a:a + chunk], U, w, with_grad=False)
        S += phi.T @ (wts[a:a + chunk, None] * phi)
    return S


# ---- V_XC ----------------------------------------------------------------------------------------------------------------------

def ao_grid(aos, pts, U=None, chunk=20000):
    """The AOs on a grid, chunk by chunk: [(start, phi, dphi), ...], to pass to vxc for several densities."""
    pts = np.asarray(pts, dtype=np.float64).reshape(3, -1)
    w_ao = ao_weights(aos)
    return [(a, *ao_on_points(aos, pts[:, a:a + chunk], U, w_ao)) for a in range(0, pts.shape[1], chunk)]


def vxc(aos, pts, wts, P, xid, cid, dfx, dfc, x_alpha=2.0 / 3.0, U=None, chunk=20000, grid=None):
    """(V_XC, n_el, E_X * dfx, E_C * dfc) of density matrix P, the quantities tf_dft_vxc returns.  grid: ao_grid's result."""
    wts = np.asarray(wts, dtype=np.float64).reshape(-1)
    P = np.asarray(P, dtype=np.float64)
    gga = xid >= X_B88 or cid >= C_LYP
    N = P.shape[0]
    A = np.zeros((N, N))
    n_el = ex = ec = 0.0
    for a, phi, dphi in (grid if grid is not None else ao_grid(aos, pts, U, chunk)):
        w = wts[a:a + phi.shape[0]]
        B = phi @ P
        rho = np.einsum("gi,gi->g", B, phi)
        grad = 2.0 * np.einsum("gi,agi->ag", B, dphi) if gga else np.zeros((3, w.size))
        rho, sigma = floors(rho, np.einsum("ag,ag->g", grad, grad))
        fx, fc, xn, xs, cn, cs = point_derivs(xid, cid, rho, sigma, x_alpha)
        vr = dfx * xn + dfc * cn
        vs = dfx * xs + dfc * cs
        D = vr[:, None] * phi
        if gga:
            D += 4.0 * vs[:, None] * np.einsum("ag,agi->gi", grad, dphi)
        A += phi.T @ (w[:, None] * D)
        n_el += float(w @ rho)
        ex += float(w @ fx)
        ec += float(w @ fc)
    return 0.5 * (A + A.T), n_el, dfx * ex, dfc * ec
