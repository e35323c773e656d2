"""TEST INFRASTRUCTURE ONLY -- an independent CPU reference of tf_dft_vxc_unrestricted (tuna_amd/csrc/tf_dft.hip.h), written from the math.

The spin-polarised counterpart of tests/xc_reference.py, whose AO evaluation, closed-shell exchange energy densities and math back
ends (NumPy for complex steps, mpmath for single points) it imports.  It imports none of the library's DFT code.  What it computes:
  * rho_s = sum P^s_ij phi_i phi_j, grad rho_s = 2 sum P^s_ij phi_i grad phi_j, floored as the kernel floors them: rho_s at 1e-23 each,
    sigma_ss = |grad rho_s|^2 at 1e-46, sigma_ab = grad rho_a . grad rho_b not floored; rho = rho_a + rho_b of the floored parts;
  * energy densities f(rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb) ONLY:
      exchange by spin scaling, f_X = (1/2) [f_x(2 rho_a, 4 sigma_aa) + f_x(2 rho_b, 4 sigma_bb)] with the closed-shell f_x of
      xc_reference (Slater, B88, B3);
      VWN5: e = e_P + alpha_c f(zeta) / f''(0) (1 - zeta^4) + (e_F - e_P) f(zeta) zeta^4 (VWN 1980, interpolation "V"), with the
      paramagnetic, ferromagnetic and spin-stiffness fits of tuna_xc.py:1631-1669 (alpha_c = -fit with A = 1 / (6 pi^2));
      VWN3: e = e_P + (e_F - e_P) f(zeta) (tuna_xc.py:1542-1600);
      LYP in the spin-resolved form of Johnson, Gill and Pople (J. Chem. Phys. 98, 5612 (1993), eq. A1);
      3P, 3P/G: 0.81 LYP + 0.19 VWN5 / VWN3;
    zeta = (rho_a - rho_b) / rho, f(zeta) = ((1 + zeta)^(4/3) + (1 - zeta)^(4/3) - 2) / (2^(4/3) - 2) with 1 +- zeta formed as
    2 rho_a / rho and 2 rho_b / rho (both floored, so zeta never leaves [-1, 1] and needs no clip).  The kernel, as the reference, forms
    zeta first: where 1 - |zeta| is below the rounding of zeta, its (1 -+ zeta)^(1/3) terms differ from this one's (VWN near zeta = +-1);
  * the five first derivatives from complex steps (NumPy) or mpmath's numerical derivative (single points) -- never from hand-derived
    formulas;
  * V^s = sym(Phi^T W (v_rho_s Phi + (4 v_sigma_ss grad rho_s + 2 v_sigma_ab grad rho_s') . grad Phi)), n_s = sum w rho_s,
    E_X,s = dfx sum w f_X,s, E_C = dfc sum w f_C.
"""
from __future__ import annotations

import numpy as np

import xc_reference as xr
from xc_reference import C_3P_VWN3, C_3P_VWN5, C_LYP, C_VWN3, C_VWN5, RHO_FLOOR, SIGMA_FLOOR, VWN3, VWN5, X_B88, _MP, _NP

VWN5_FERRO = (-0.32500, 7.06042, 18.0578, 0.01554535)
VWN3_FERRO = (-0.743294, 20.1231, 101.578, 0.01554535)
VWN5_STIFF = (-0.0047584, 1.13107, 13.0045, None)          # A = 1 / (6 pi^2)


def _e_vwn(M, n, params):
    """VWN energy per particle of one fit (x0, b, c, A) at total density n."""
    x0, b, c, A = params
    if A is None:
        A = 1.0 / (6.0 * M.pi * M.pi)
    Q = (4.0 * c - b * b) ** 0.5
    X0 = x0 * x0 + b * x0 + c
    c1 = -b * x0 / X0
    c2 = 2.0 * b * (c - x0 * x0) / (Q * X0)
    rs = M.cbrt(3.0 / (4.0 * M.pi * n))
    x = M.sqrt(rs)
    Xx = rs + b * x + c
    return A * (M.log(rs / Xx) + c1 * M.log((x - x0) * (x - x0) / Xx) + c2 * M.atan(Q / (2.0 * x + b)))


def _fz(M, na, nb):
    """f(zeta) from 1 + zeta = 2 rho_a / rho and 1 - zeta = 2 rho_b / rho: analytic for rho_a, rho_b > 0 (both are floored), so the
    complex step is exact up to zeta = +-1, where (1 -+ zeta)^(4/3) formed from a rounded zeta is not."""
    n = na + nb
    return (M.cbrt(2.0 * na / n) ** 4 + M.cbrt(2.0 * nb / n) ** 4 - 2.0) / (M.cbrt(2.0) ** 4 - 2.0)


def vwn5_spin(M, na, nb):
    n = na + nb
    z = (na - nb) / n
    eP, eF, ac = _e_vwn(M, n, VWN5), _e_vwn(M, n, VWN5_FERRO), -_e_vwn(M, n, VWN5_STIFF)
    fpp0 = 8.0 / (9.0 * (M.cbrt(2.0) ** 4 - 2.0))
    f, z4 = _fz(M, na, nb), z ** 4
    return n * (eP + ac * f / fpp0 * (1.0 - z4) + (eF - eP) * f * z4)


def vwn3_spin(M, na, nb):
    n = na + nb
    eP, eF = _e_vwn(M, n, VWN3), _e_vwn(M, n, VWN3_FERRO)
    return n * (eP + (eF - eP) * _fz(M, na, nb))


def lyp_spin(M, na, nb, saa, sab, sbb):
    """Johnson-Gill-Pople eq. A1."""
    a, b, c, d = 0.04918, 0.132, 0.2533, 0.349
    n = na + nb
    icn = 1.0 / M.cbrt(n)
    omega = M.exp(-c * icn) / (1.0 + d * icn) * icn ** 11
    delta = c * icn + d * icn / (1.0 + d * icn)
    CF = 3.0 / 10.0 * M.cbrt(3.0 * M.pi * M.pi) ** 2
    g2 = saa + sbb + 2.0 * sab
    # the last three terms of eq. A1, -2/3 n^2 g2 + (2/3 n^2 - na^2) sbb + (2/3 n^2 - nb^2) saa, collected: written as in the paper they
    # cancel to the rounding of n^2 sigma, which swamps the whole bracket when one spin density is on the floor
    bracket = (na * nb * (M.cbrt(2.0) ** 11 * CF * (M.cbrt(na) ** 8 + M.cbrt(nb) ** 8) + (47.0 / 18.0 - 7.0 * delta / 18.0) * g2
                          - (5.0 / 2.0 - delta / 18.0) * (saa + sbb) - (delta - 11.0) / 9.0 * (na / n * saa + nb / n * sbb))
               - 4.0 / 3.0 * n * n * sab - na * na * sbb - nb * nb * saa)
    return -4.0 * a / (1.0 + d * icn) * na * nb / n - a * b * omega * bracket


def f_x_spin(M, xid, na, nb, saa, sbb, x_alpha):
    """(f_X,alpha, f_X,beta): exchange of each spin by the spin-scaling relation."""
    return 0.5 * xr.f_x(M, xid, 2.0 * na, 4.0 * saa, x_alpha), 0.5 * xr.f_x(M, xid, 2.0 * nb, 4.0 * sbb, x_alpha)


def f_c_spin(M, cid, na, nb, saa, sab, sbb):
    if cid == C_VWN5:
        return vwn5_spin(M, na, nb)
    if cid == C_VWN3:
        return vwn3_spin(M, na, nb)
    if cid == C_LYP:
        return lyp_spin(M, na, nb, saa, sab, sbb)
    if cid in (C_3P_VWN5, C_3P_VWN3):
        return 0.81 * lyp_spin(M, na, nb, saa, sab, sbb) + 0.19 * (vwn5_spin(M, na, nb) if cid == C_3P_VWN5 else vwn3_spin(M, na, nb))
    return 0.0 * na


def _total(M, xid, cid, dfx, dfc, x_alpha, v):
    na, nb, saa, sab, sbb = v
    fa, fb = f_x_spin(M, xid, na, nb, saa, sbb, x_alpha)
    return dfx * (fa + fb) + dfc * f_c_spin(M, cid, na, nb, saa, sab, sbb)


def point_derivs(xid, cid, dfx, dfc, na, nb, saa, sab, sbb, x_alpha=2.0 / 3.0):
    """Complex-step (f_X,a, f_X,b, f_C, d f / d (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb)) of f = dfx f_X + dfc f_C on arrays of
    floored points; f_X and f_C unscaled."""
    v = [np.asarray(x, dtype=np.float64) for x in (na, nb, saa, sab, sbb)]
    scale = np.maximum(np.sqrt(v[2] * v[4]), 1e-200)
    fa, fb = f_x_spin(_NP, xid, v[0], v[1], v[2], v[4], x_alpha)
    fc = f_c_spin(_NP, cid, v[0], v[1], v[2], v[3], v[4])
    ones = np.ones_like(v[0])
    der = []
    for k in range(5):
        h = 1e-30 * (np.maximum(np.abs(v[k]), scale) if k == 3 else v[k])
        w = [x.astype(complex) for x in v]
        w[k] = w[k] + 1j * h
        der.append(np.imag(_total(_NP, xid, cid, dfx, dfc, x_alpha, w)) / h * ones)
    return np.real(fa) * ones, np.real(fb) * ones, np.real(fc) * ones, der


def mp_point(xid, cid, dfx, dfc, na, nb, saa, sab, sbb, x_alpha=2.0 / 3.0, dps=40):
    """(f, df/drho_a, df/drho_b, df/dsigma_aa, df/dsigma_ab, df/dsigma_bb) of f = dfx f_X + dfc f_C at ONE floored point with mpmath."""
    import mpmath
    M = _MP()
    with mpmath.workdps(dps + 20):
        v = [mpmath.mpf(float(x)) for x in (na, nb, saa, sab, sbb)]
        pars = [mpmath.mpf(float(x)) for x in (dfx, dfc, x_alpha)]
        f = lambda w: _total(M, xid, cid, pars[0], pars[1], pars[2], w)   # noqa: E731
        out = [f(v)]
        for k in range(5):
            h = (abs(v[k]) if v[k] != 0 else mpmath.sqrt(v[2] * v[4])) * mpmath.mpf(10) ** -15

            def g(t, k=k):
                w = list(v)
                w[k] = t
                return f(w)
            out.append(mpmath.diff(g, v[k], h=h))
        return tuple(float(x) for x in out)


def floors(ra, rb, ga, gb):
    ra, rb = np.maximum(ra, RHO_FLOOR), np.maximum(rb, RHO_FLOOR)
    saa = np.maximum(np.einsum("ag,ag->g", ga, ga), SIGMA_FLOOR)
    sbb = np.maximum(np.einsum("ag,ag->g", gb, gb), SIGMA_FLOOR)
    return ra, rb, saa, np.einsum("ag,ag->g", ga, gb), sbb


def vxc_unrestricted(aos, pts, wts, Pa, Pb, xid, cid, dfx, dfc, x_alpha=2.0 / 3.0, U=None, chunk=20000, grid=None):
    """(V^alpha, V^beta, (n_alpha, n_beta), (E_X,alpha * dfx, E_X,beta * dfx), E_C * dfc): what tf_dft_vxc_unrestricted returns."""
    wts = np.asarray(wts, dtype=np.float64).reshape(-1)
    Pa, Pb = np.asarray(Pa, dtype=np.float64), np.asarray(Pb, dtype=np.float64)
    gga = xid >= X_B88 or cid >= C_LYP
    N = Pa.shape[0]
    Aa, Ab = np.zeros((N, N)), np.zeros((N, N))
    n = np.zeros(2)
    ex = np.zeros(2)
    ec = 0.0
    for a, phi, dphi in (grid if grid is not None else xr.ao_grid(aos, pts, U, chunk)):
        w = wts[a:a + phi.shape[0]]
        Ba, Bb = phi @ Pa, phi @ Pb
        ra, rb = np.einsum("gi,gi->g", Ba, phi), np.einsum("gi,gi->g", Bb, phi)
        ga = 2.0 * np.einsum("gi,agi->ag", Ba, dphi) if gga else np.zeros((3, w.size))
        gb = 2.0 * np.einsum("gi,agi->ag", Bb, dphi) if gga else np.zeros((3, w.size))
        ra, rb, saa, sab, sbb = floors(ra, rb, ga, gb)
        fa, fb, fc, (va, vb, vaa, vab, vbb) = point_derivs(xid, cid, dfx, dfc, ra, rb, saa, sab, sbb, x_alpha)
        Da, Db = va[:, None] * phi, vb[:, None] * phi
        if gga:
            ca = 4.0 * vaa * ga + 2.0 * vab * gb
            cb = 4.0 * vbb * gb + 2.0 * vab * ga
            Da += np.einsum("ag,agi->gi", ca, dphi)
            Db += np.einsum("ag,agi->gi", cb, dphi)
        Aa += phi.T @ (w[:, None] * Da)
        Ab += phi.T @ (w[:, None] * Db)
        n += [float(w @ ra), float(w @ rb)]
        ex += [float(w @ fa), float(w @ fb)]
        ec += float(w @ fc)
    return 0.5 * (Aa + Aa.T), 0.5 * (Ab + Ab.T), (float(n[0]), float(n[1])), (dfx * float(ex[0]), dfx * float(ex[1])), dfc * ec
