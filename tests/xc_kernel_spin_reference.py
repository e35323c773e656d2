"""Independent NumPy model of the spin-resolved exchange-correlation kernel of unrestricted TD-DFT / TDA and of the Kohn-Sham stability
analysis for the local-density functionals (no library code): what tf_xc_kernel_uhf, tf_tddft_uhf and tf_stability_uks compute, with
the conventions written out once.

Point kernels, per grid point, from rho_a and rho_b floored at 1e-23 EACH, n = rho_a + rho_b of the floored values, with F the energy
density per volume (E = int F):
    f_X,ss = d2 F_X / d rho_s^2 = 2 f(2 rho_s),   f(m) = -(alpha / 2) (3 / pi)^(1/3) m^(-2/3)  the bare Slater second derivative
             (E_X[rho_a, rho_b] = (E_X[2 rho_a] + E_X[2 rho_b]) / 2);   f_X,ab = 0
    f_C,st = d2 (n e_C(n, zeta)) / d rho_s d rho_t through the chain rule from (n, zeta), zeta = (rho_a - rho_b) / n clipped to [-1, 1]:
             f_nn = (r_s^2 e_rr - 2 r_s e_r) / (9 n),  f_nz = e_z - (r_s / 3) e_rz,  f_zz = n e_zz,  f_z = n e_z,
             zeta_a = (1 - zeta) / n,  zeta_b = -(1 + zeta) / n,  zeta_aa = -2 (1 - zeta) / n^2,  zeta_bb = 2 (1 + zeta) / n^2,  zeta_ab = 2 zeta / n^2,
             f_st = f_nn + f_nz (zeta_s + zeta_t) + f_zz zeta_s zeta_t + f_z zeta_st
    VWN3: e = e_0 + (e_1 - e_0) f(zeta);   VWN5: e = e_0 (1 - h) + e_1 h + alpha_c g,  h = f zeta^4,  g = f (1 - zeta^4) / f''(0),
    f(zeta) the spin-scaling function, f''(zeta) with 1 +- zeta floored at 1e-23.
At zeta = 0: f_aa + f_ab and f_aa - f_ab are the restricted singlet and triplet kernels of xc_kernel_reference.py.

Every point function returns the value and "mag", an upper bound of the sum of the magnitudes of the terms of its closed form, carried
through the arithmetic by the class V below: mag(a + b) = mag a + mag b, mag(a b) = mag a mag b, mag(a / b) = mag a mag b / b^2.  zeta
and 1 +- zeta count as exact inputs (one correctly rounded division and a subtraction of it from 1 that both sides do alike); a fit's
e, e', e'' carry the magnitudes of xc_kernel_reference._vwn_fit.  A result computed with other roundings of the same operations
differs by a few roundings of mag, not of the value: the bound of the GPU test is POINT_TOL = 64 eps of mag, as for the restricted
kernels.

Matrix, in the compound index of tf_cis_uhf (alpha block (ia) = i v_a + a, then the beta block):
    K[p][q] = sum_g u_st(g) psi_i^s psi_a^s psi_j^t psi_b^t,   u_ss = w (DFX f_X,ss + DFC f_C,ss),   u_ab = w DFC f_C,ab."""
from __future__ import annotations

import numpy as np

import xc_kernel_reference as xk

FLOOR = 1e-23
EPS = np.finfo(np.float64).eps
POINT_TOL = 64 * EPS
DEN = np.cbrt(2.0) ** 4 - 2.0
VWN5_FERRO = (-0.32500, 7.06042, 18.0578, 0.01554535)


class V:
    """a value with an upper bound of the sum of the magnitudes of the terms it was formed from"""
    __array_ufunc__ = None                                    # ndarray * V goes to V.__rmul__

    def __init__(self, v, m=None):
        self.v = np.asarray(v, float)
        self.m = np.abs(self.v) if m is None else np.asarray(m, float)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.m)

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.m * o.m)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        return V(self.v / o.v, self.m * o.m / (o.v * o.v))


def slater_bare(m, x_alpha=2.0 / 3.0):
    """the bare second derivative of m e_X(m) (one term)"""
    return -(x_alpha / 2.0) * np.cbrt(3.0 / np.pi) * np.cbrt(m) ** -2.0


def zeta_of(ra, rb):
    return np.clip((ra - rb) / (ra + rb), -1.0, 1.0)


def spin_scaling(z):
    """f, f', f'' of zeta as V"""
    p, m = np.cbrt(1 + z), np.cbrt(1 - z)
    f = V((p ** 4 + m ** 4 - 2) / DEN, (p ** 4 + m ** 4 + 2) / DEN)
    fp = V((p - m) / DEN * 4 / 3, (p + m) / DEN * 4 / 3)
    pf, mf = np.cbrt(np.maximum(1 + z, FLOOR)), np.cbrt(np.maximum(1 - z, FLOOR))
    fpp = V((4 / 9) * (pf ** -2.0 + mf ** -2.0) / DEN)
    return f, fp, fpp


def _fit(n, params):
    d = xk._vwn_fit(n, params)
    return V(d["e"], d["e_mag"]), V(d["de"], d["de_mag"]), V(d["d2e"], d["d2e_mag"]), d["r_s"]


def _chain(n, z, r_s, e_r, e_rr, e_z, e_zz, e_rz):
    f_nn = (r_s * r_s * e_rr - 2 * r_s * e_r) / (9 * n)
    f_nz = e_z - (r_s / 3) * e_rz
    f_zz = n * e_zz
    f_z = n * e_z
    zu, zw = (1 - z) / n, -(1 + z) / n
    zuu, zww, zuw = -2 * (1 - z) / n ** 2, 2 * (1 + z) / n ** 2, 2 * z / n ** 2
    faa = f_nn + 2 * f_nz * zu + f_zz * (zu * zu) + f_z * zuu
    fbb = f_nn + 2 * f_nz * zw + f_zz * (zw * zw) + f_z * zww
    fab = f_nn + f_nz * (zu + zw) + f_zz * (zu * zw) + f_z * zuw
    return faa, fab, fbb


def vwn_spin(ra, rb, which):
    """(f_C,aa, f_C,ab, f_C,bb) as V of "VWN3" or "VWN5" at floored spin densities"""
    n = ra + rb
    z = zeta_of(ra, rb)
    f, fp, fpp = spin_scaling(z)
    if which == "VWN3":
        (e0, d0, dd0, r_s), (e1, d1, dd1, _) = _fit(n, xk.VWN3_PARA), _fit(n, xk.VWN3_FERRO)
        e_r = d0 * (1 - f) + d1 * f
        e_rr = dd0 * (1 - f) + dd1 * f
        e_z, e_zz, e_rz = (e1 - e0) * fp, (e1 - e0) * fpp, (d1 - d0) * fp
        return _chain(n, z, r_s, e_r, e_rr, e_z, e_zz, e_rz)
    (e0, d0, dd0, r_s), (e1, d1, dd1, _), (ea, da, dda, _) = _fit(n, xk.VWN5_PARA), _fit(n, VWN5_FERRO), _fit(n, xk.VWN5_STIFF)
    al, dal, ddal = -ea, -da, -dda
    z2, z3, z4 = z * z, z * z * z, z * z * z * z
    h, hp, hpp = f * z4, fp * z4 + 4 * f * z3, fpp * z4 + 8 * fp * z3 + 12 * f * z2
    g, gp = f * (1 - z4) / xk.FPP0, (fp * (1 - z4) - 4 * f * z3) / xk.FPP0
    gpp = (fpp * (1 - z4) - 8 * fp * z3 - 12 * f * z2) / xk.FPP0
    e_r = d0 * (1 - h) + d1 * h + dal * g
    e_rr = dd0 * (1 - h) + dd1 * h + ddal * g
    e_z, e_zz = (e1 - e0) * hp + al * gp, (e1 - e0) * hpp + al * gpp
    e_rz = (d1 - d0) * hp + dal * gp
    return _chain(n, z, r_s, e_r, e_rr, e_z, e_zz, e_rz)


def point_kernels(rho_a, rho_b, functional, x_alpha=2.0 / 3.0, floored=False):
    """{"rho_a", "rho_b" (floored), "f_X_aa", "f_X_bb", "f_C_aa", "f_C_ab", "f_C_bb", "mag_<each>", "dfx", "dfc", "hfx"} on arrays of raw spin
    densities"""
    xn, cn, dfx, hfx, dfc = xk.FUNCTIONALS[functional.upper()]
    ra, rb = (np.asarray(x, float) if floored else np.maximum(np.asarray(x, float), FLOOR) for x in (rho_a, rho_b))
    zero = np.zeros_like(ra)
    out = dict(rho_a=ra, rho_b=rb, dfx=dfx, dfc=dfc, hfx=hfx)
    for s, r in (("aa", ra), ("bb", rb)):
        out["f_X_" + s] = 2.0 * slater_bare(2.0 * r, x_alpha) if xn == "S" else zero
        out["mag_f_X_" + s] = np.abs(out["f_X_" + s])
    if cn:
        with np.errstate(all="ignore"):
            faa, fab, fbb = vwn_spin(ra, rb, cn)
        for s, f in (("aa", faa), ("ab", fab), ("bb", fbb)):
            out["f_C_" + s], out["mag_f_C_" + s] = f.v, f.m
    else:
        for s in ("aa", "ab", "bb"):
            out["f_C_" + s] = out["mag_f_C_" + s] = zero
    return out


def weights_u(w, pk):
    """(u_aa, u_ab, u_bb) and the sums of the magnitudes of their terms"""
    u = [w * (pk["dfx"] * pk["f_X_aa"] + pk["dfc"] * pk["f_C_aa"]), w * (pk["dfc"] * pk["f_C_ab"]), w * (pk["dfx"] * pk["f_X_bb"] + pk["dfc"] * pk["f_C_bb"])]
    aw = np.abs(w)
    m = [aw * (pk["dfx"] * pk["mag_f_X_aa"] + pk["dfc"] * pk["mag_f_C_aa"]), aw * (pk["dfc"] * pk["mag_f_C_ab"]),
         aw * (pk["dfx"] * pk["mag_f_X_bb"] + pk["dfc"] * pk["mag_f_C_bb"])]
    return u, m


def transition_densities(psi_oa, psi_va, psi_ob, psi_vb):
    """(T_alpha [d_a, G], T_beta [d_b, G]) = psi_i psi_a per spin; a spin without rows gives [0, G]"""
    out = []
    for po, pv in ((psi_oa, psi_va), (psi_ob, psi_vb)):
        po, pv = np.asarray(po, float), np.asarray(pv, float)
        G = max(po.shape[-1] if po.ndim == 2 else 0, pv.shape[-1] if pv.ndim == 2 else 0)
        if po.size == 0 or pv.size == 0:
            out.append(np.zeros((0, G)))
        else:
            out.append((po[:, None, :] * pv[None, :, :]).reshape(-1, po.shape[1]))
    G = max(t.shape[1] for t in out)
    return [t if t.shape[1] == G else np.zeros((0, G)) for t in out]


def spin_kernel_matrix(psi_oa, psi_va, psi_ob, psi_vb, u_aa, u_ab, u_bb, with_magnitudes=False, mags=None):
    """K [d_a + d_b, d_a + d_b] in the library's order; with_magnitudes also S, the sum of the magnitudes of the terms (with mags = the
    three magnitude vectors in place of |u|)"""
    Ta, Tb = transition_densities(psi_oa, psi_va, psi_ob, psi_vb)
    return blocks_from(Ta, Tb, (u_aa, u_ab, u_bb), with_magnitudes, mags)


def blocks_from(Ta, Tb, u, with_magnitudes=False, mags=None):
    def build(Ta, Tb, u):
        return np.block([[(Ta * u[0]) @ Ta.T, (Ta * u[1]) @ Tb.T], [(Tb * u[1]) @ Ta.T, (Tb * u[2]) @ Tb.T]])
    K = build(Ta, Tb, u)
    if not with_magnitudes:
        return K
    return K, build(np.abs(Ta), np.abs(Tb), [np.abs(x) for x in (u if mags is None else mags)])


def spin_windows(C_alpha, C_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0):
    Ca, Cb = np.asarray(C_alpha, float), np.asarray(C_beta, float)
    return (Ca[:, n_frozen_alpha:n_alpha], Ca[:, n_alpha:]), (Cb[:, n_frozen_beta:n_beta], Cb[:, n_beta:])


def model_kernel(phi, w, functional, C_alpha, C_beta, P_alpha, P_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0):
    """The model's K on a grid (phi [G, N], w [G]) with what its bound needs: {"K", "S" (sum of the magnitudes of the terms u T T, u by the
    magnitudes of ITS terms), "D" (the first-order change of K when either rho_s(g) moves by one unit of its rho_mag_s(g), summed in
    magnitude; RHO_TOL times this is what densities within RHO_TOL rho_mag can change), "rho", "rho_mag" [2, G], "pk", "u", "G"}."""
    (Coa, Cva), (Cob, Cvb) = spin_windows(C_alpha, C_beta, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta)
    rho, mag = zip(xk.density(phi, P_alpha), xk.density(phi, P_beta))
    pk = point_kernels(rho[0], rho[1], functional)
    u, m = weights_u(w, pk)
    Ta, Tb = transition_densities((phi @ Coa).T, (phi @ Cva).T, (phi @ Cob).T, (phi @ Cvb).T)
    K, S = blocks_from(Ta, Tb, u, True, m)
    h = 1e-4
    D = np.zeros_like(K)
    ra, rb = pk["rho_a"], pk["rho_b"]
    for s in range(2):                                        # d u / d ln rho_s by a central difference of the closed forms
        fa = (1 + h, 1 - h) if s == 0 else (1, 1)
        fb = (1 + h, 1 - h) if s == 1 else (1, 1)
        up, _ = weights_u(w, point_kernels(ra * fa[0], rb * fb[0], functional))
        dn, _ = weights_u(w, point_kernels(ra * fa[1], rb * fb[1], functional))
        amp = np.where(rho[s] > FLOOR, mag[s] / pk["rho_" + "ab"[s]], 0.0)
        D += blocks_from(np.abs(Ta), np.abs(Tb), [np.abs(a - b) / (2 * h) * amp for a, b in zip(up, dn)])
    return dict(K=K, S=S, D=D, rho=np.array([ra, rb]), rho_mag=np.array(mag), pk=pk, u=u, G=len(w))


def k_bound(m):
    """per element: two float64 sums of G terms in any order, plus what densities within RHO_TOL of the sums of their terms' magnitudes move"""
    return 2 * xk.gamma(m["G"]) * m["S"] + xk.RHO_TOL * m["D"]


def matrices(E, C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, hfx, K=None):
    """{"A", "B", "plus", "minus"} [dim, dim], alpha block first: ucis_reference.matrices with the exchange blocks scaled by hfx and K added
    (before the symmetrisation, as the reference): A = d_st (Delta - hfx H) + G + K, B = -d_st hfx X + G + K."""
    from mp3_reference import _windows, mo_tensor
    w = [_windows(C_alpha, eps_alpha, n_alpha, n_frozen_alpha), _windows(C_beta, eps_beta, n_beta, n_frozen_beta)]
    d = [Co.shape[1] * Cv.shape[1] for Co, Cv, _, _ in w]
    off, dim = [0, d[0]], d[0] + d[1]
    A, B = np.zeros((dim, dim)), np.zeros((dim, dim))
    for s, (Co, Cv, eo, ev) in enumerate(w):
        if d[s] == 0:
            continue
        sl = slice(off[s], off[s] + d[s])
        ovov = mo_tensor(E, Co, Cv, Co, Cv)
        G = ovov.reshape(d[s], d[s])
        X = ovov.transpose(0, 3, 2, 1).reshape(d[s], d[s])
        H = mo_tensor(E, Co, Co, Cv, Cv).transpose(0, 2, 1, 3).reshape(d[s], d[s]) if hfx != 0 else 0.0
        A[sl, sl] = np.diag((ev[None, :] - eo[:, None]).ravel()) + G - hfx * H
        B[sl, sl] = G - hfx * X
    if d[0] and d[1]:
        G = mo_tensor(E, w[0][0], w[0][1], w[1][0], w[1][1]).reshape(d[0], d[1])
        for M in (A, B):
            M[:d[0], d[0]:] = G
            M[d[0]:, :d[0]] = G.T
    if K is not None:
        A, B = A + K, B + K
    A, B = 0.5 * (A + A.T), 0.5 * (B + B.T)
    return {"A": A, "B": B, "plus": A + B, "minus": A - B}


# ---- the systems of tests/golden/utddft_systems.npz (tools/make_golden_utddft.py) and their grids rebuilt ---------------------------

# tag -> (symbols, R in angstrom or None, basis, n_alpha, n_beta, functional, grid)
SYSTEMS = {
    "nh_hfs_sto3g": (["N", "H"], 1.036, "STO-3G", 5, 3, "HFS", "loose"),
    "nh_svwn3_sto3g": (["N", "H"], 1.036, "STO-3G", 5, 3, "SVWN3", "loose"),
    "li_svwn3_631g": (["LI"], None, "6-31G", 2, 1, "SVWN3", "loose"),
    "oh_lda_sto3g": (["O", "H"], 0.9697, "STO-3G", 5, 4, "SVWN", "loose"),
    "lih_cation_lda_631g": (["LI", "H"], 1.595, "6-31G", 2, 1, "SVWN", "loose"),
    "h_lda_631g": (["H"], None, "6-31G", 1, 0, "SVWN", "loose"),
    "lih_stretched_lda_sto3g": (["LI", "H"], 4.0, "STO-3G", 2, 2, "SVWN", "loose"),         # unstable: the restricted solution past the
    "h2_stretched_svwn3_sto3g": (["H", "H"], 3.0, "STO-3G", 1, 1, "SVWN3", "loose"),         # spin-symmetry breaking point
}
UNSTABLE = ("lih_stretched_lda_sto3g", "h2_stretched_svwn3_sto3g")
_REBUILT = {}


def frozen_variants(g):
    """frozen spin orbitals of the stored variants: one orbital per spin where o_beta > 1"""
    return (0, 2) if int(g["n_beta"]) > 1 else (0,)


def stable(g, k=0):
    return f"TDDFT_fc{k}_energies" in g and f"TDA_fc{k}_energies" in g


def system(tag):
    from tuna_amd import molecule as mol
    sym, R, basis, na, nb, functional, grid = SYSTEMS[tag]
    atoms = mol.make_atoms(sym, None if R is None else mol.angstrom_to_bohr(R))
    shells = mol.build_shells(atoms, basis)
    return atoms, shells, mol.expand_cartesian_aos(shells)


def rebuilt(tag):
    """as xc_kernel_reference.rebuilt, for the open-shell systems"""
    if tag not in _REBUILT:
        import xc_reference as xr
        from tuna_amd import dft
        from tuna_amd.spherical import transformation_matrix
        atoms, shells, aos = system(tag)
        pts, wts, _ = dft.integration_grid(atoms, SYSTEMS[tag][6])
        pts, wts = np.asarray(pts, float).reshape(3, -1), np.asarray(wts, float).reshape(-1)
        phi, _ = xr.ao_on_points(aos, pts, transformation_matrix([s.L for s in shells]), with_grad=False)
        _REBUILT[tag] = dict(atoms=atoms, shells=shells, aos=aos, pts=pts, wts=wts, phi=phi)
    return _REBUILT[tag]


def golden_model(tag, g, k=0):
    r = rebuilt(tag)
    return model_kernel(r["phi"], r["wts"], SYSTEMS[tag][5], g["C_alpha"], g["C_beta"], g["P_alpha"], g["P_beta"], int(g["n_alpha"]), int(g["n_beta"]),
                        k // 2, k // 2)
