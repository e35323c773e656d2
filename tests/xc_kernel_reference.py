"""Independent NumPy model of closed-shell TD-DFT / TDA for the local-density functionals (no library code): what tf_xc_kernel_rhf and
tf_tddft_rhf compute, with the conventions written out once.

Point kernels, per grid point, from the floored density n (floor 1e-23), with f = n e the energy density per volume:
    f_X   = 2 d2(n e_X)/dn2          Slater: d2f/dn2 = -(alpha / 2) (3 / pi)^(1/3) n^(-2/3)
    f_C^S = 2 d2(n e_C)/dn2          VWN, with r_s = (3 / (4 pi n))^(1/3), x = sqrt(r_s):
                                        VWN3 form: d2f/dn2 = (r_s^2 e'' - 2 r_s e') / (9 n),        e' = de/dr_s
                                        VWN5 form: d2f/dn2 = x A / (36 n) (x dcombo/dx - 5 combo)   (the same function of the fit)
    f_C^T = 2 f_mm                   VWN3: f_mm = f''(0) (e_ferro - e_para) / n,   VWN5: f_mm = alpha_c / n  (the spin-stiffness fit)
so that f^S = f_aa + f_ab and f^T = f_aa - f_ab of the spin-resolved second derivatives at zero polarisation.  Every function returns
the value and the sum of the magnitudes of the terms of its closed form ("mag"), every logarithm of a quotient counted as the two
logarithms it is the difference of: the terms of the VWN forms cancel by orders of magnitude -- the rational terms of d2f/dn2 at high
density, log r_s against log X at low density, where r_s / X -> 1 -- and a result computed with other roundings of the same operations
differs by a few roundings of that sum, not of the value.

Matrices:  K[(ia)][(jb)] = sum_g u(g) psi_i psi_a psi_j psi_b,  u_S = w (DFX f_X + DFC f_C^S),  u_T = w (DFX f_X + DFC f_C^T);
    singlet A = Delta + 2 (ia|jb) - hfx (ij|ab) + K_S,  B = 2 (ia|jb) - hfx (ib|ja) + K_S
    triplet A = Delta - hfx (ij|ab) + K_T,              B = -hfx (ib|ja) + K_T
each symmetrised; TDA = eigh(A); full = the reference's route, the positive roots of [[A, B], [-B, -A]] (cis_reference.tdhf_full)."""
from __future__ import annotations

import numpy as np

import cis_reference as cr
from mp3_reference import _windows, mo_tensor

FLOOR = 1e-23
VWN5_PARA = (-0.10498, 3.72744, 12.9352, 0.0310907)
VWN3_PARA = (-0.409286, 13.0720, 42.7198, 0.0310907)
VWN3_FERRO = (-0.743294, 20.1231, 101.578, 0.01554535)
VWN5_STIFF = (-0.0047584, 1.13107, 13.0045, 1.0 / (6.0 * np.pi ** 2))
FPP0 = 8.0 / (9.0 * (np.cbrt(2.0) ** 4 - 2.0))
# functional name -> (exchange, correlation, DFX, HFX, DFC)
FUNCTIONALS = {"HFS": ("S", None, 1.0, 0.0, 0.0), "SVWN": ("S", "VWN5", 1.0, 0.0, 1.0), "LDA": ("S", "VWN5", 1.0, 0.0, 1.0),
               "LSDA": ("S", "VWN5", 1.0, 0.0, 1.0), "SVWN5": ("S", "VWN5", 1.0, 0.0, 1.0), "SVWN3": ("S", "VWN3", 1.0, 0.0, 1.0)}


def slater_fx(n, x_alpha=2.0 / 3.0):
    """(f_X, mag): one term"""
    f = 2.0 * (-(x_alpha / 2.0) * np.cbrt(3.0 / np.pi) * np.cbrt(n) ** -2.0)
    return f, np.abs(f)


def _vwn_fit(n, params):
    """e, e' = de/dr_s, e'' and combo, dcombo/dx of one fit, each with the sum of the magnitudes of its terms"""
    x_0, b, c, A = params
    Q = np.sqrt(4 * c - b * b)
    X_0 = x_0 * x_0 + b * x_0 + c
    c_1 = -b * x_0 / X_0
    c_2 = 2 * b * (c - x_0 * x_0) / (Q * X_0)
    r_s = np.cbrt(3.0 / (4.0 * np.pi * n))
    x = np.sqrt(r_s)
    xm = x - x_0
    X = r_s + b * x + c
    t_e = [np.log(r_s / X), c_1 * np.log(xm * xm / X), c_2 * np.arctan(Q / (2 * x + b))]
    t_c = [2 / x, 2 * c_1 / xm, -(2 * x + b) * (1 + c_1) / X, -0.5 * c_2 * Q / X]
    t_d = [-2 / r_s, -2 * c_1 / (xm * xm), -2 * (1 + c_1) / X, (2 * x + b) ** 2 * (1 + c_1) / (X * X), 0.5 * c_2 * Q * (2 * x + b) / (X * X)]
    # the magnitudes behind e: a logarithm of a quotient is the difference of two logarithms -- rounding the quotient by eps moves it by
    # eps however small it is, which is that cancellation (at low density r_s / X -> 1: log r_s and log X agree to 1e-4 of themselves)
    m_e = [np.abs(np.log(r_s)) + np.abs(np.log(X)), np.abs(c_1) * (np.abs(np.log(xm * xm)) + np.abs(np.log(X))), np.abs(t_e[2])]
    e, e_mag = A * sum(t_e), A * sum(m_e)
    combo, combo_mag = sum(t_c), sum(np.abs(t) for t in t_c)
    dcombo, dcombo_mag = sum(t_d), sum(np.abs(t) for t in t_d)
    return dict(A=A, r_s=r_s, x=x, e=e, e_mag=e_mag, combo=combo, combo_mag=combo_mag, dcombo=dcombo, dcombo_mag=dcombo_mag,
                de=(A / 2) * combo / x, de_mag=(A / 2) * combo_mag / x,
                d2e=A * (x * dcombo - combo) / (4 * x ** 3), d2e_mag=A * (x * dcombo_mag + combo_mag) / (4 * x ** 3))


def vwn_fc(n, which):
    """(f_C^S, mag_S, f_C^T, mag_T) of "VWN5" or "VWN3" """
    if which == "VWN3":
        p, q = _vwn_fit(n, VWN3_PARA), _vwn_fit(n, VWN3_FERRO)
        r = p["r_s"]
        fS = 2.0 * (r * r * p["d2e"] - 2 * r * p["de"]) / (9 * n)
        mS = 2.0 * (r * r * p["d2e_mag"] + 2 * r * p["de_mag"]) / (9 * n)
        fT = 2.0 * FPP0 * (q["e"] - p["e"]) / n
        mT = 2.0 * FPP0 * (q["e_mag"] + p["e_mag"]) / n
        return fS, mS, fT, mT
    p, s = _vwn_fit(n, VWN5_PARA), _vwn_fit(n, VWN5_STIFF)
    x = p["x"]
    fS = 2.0 * (x * p["A"]) / (36 * n) * (x * p["dcombo"] - 5 * p["combo"])
    mS = 2.0 * (x * p["A"]) / (36 * n) * (x * p["dcombo_mag"] + 5 * p["combo_mag"])
    return fS, mS, 2.0 * (-s["e"]) / n, 2.0 * s["e_mag"] / n


def point_kernels(rho, functional, x_alpha=2.0 / 3.0):
    """{"rho" (floored), "f_X", "f_CS", "f_CT", "mag_X", "mag_CS", "mag_CT", "dfx", "dfc", "hfx"} on an array of raw densities"""
    xn, cn, dfx, hfx, dfc = FUNCTIONALS[functional.upper()]
    n = np.maximum(np.asarray(rho, float), FLOOR)
    zero = np.zeros_like(n)
    fX, mX = slater_fx(n, x_alpha) if xn == "S" else (zero, zero)
    fS, mS, fT, mT = vwn_fc(n, cn) if cn else (zero, zero, zero, zero)
    return dict(rho=n, f_X=fX, f_CS=fS, f_CT=fT, mag_X=mX, mag_CS=mS, mag_CT=mT, dfx=dfx, dfc=dfc, hfx=hfx)


def weights_u(w, pk):
    """(u_S, u_T) and the sums of the magnitudes of their terms"""
    uS, uT = w * (pk["dfx"] * pk["f_X"] + pk["dfc"] * pk["f_CS"]), w * (pk["dfx"] * pk["f_X"] + pk["dfc"] * pk["f_CT"])
    mS = np.abs(w) * (pk["dfx"] * pk["mag_X"] + pk["dfc"] * pk["mag_CS"])
    mT = np.abs(w) * (pk["dfx"] * pk["mag_X"] + pk["dfc"] * pk["mag_CT"])
    return uS, uT, mS, mT


def transition_density(phi, C, n_occ, n_frozen=0):
    """T [dim, G] = psi_i psi_a from the AOs on the grid phi [G, N]"""
    Co, Cv = np.asarray(C, float)[:, n_frozen:n_occ], np.asarray(C, float)[:, n_occ:]
    po, pv = (phi @ Co).T, (phi @ Cv).T
    return (po[:, None, :] * pv[None, :, :]).reshape(-1, phi.shape[0])


def kernel_matrix(T, u, mag=None):
    """K = sum_g u T T (and, with mag, the sum of the magnitudes of the terms with |u| replaced by mag)"""
    K = (T * u) @ T.T
    return K if mag is None else (K, (np.abs(T) * mag) @ np.abs(T).T)


def matrices(E, C, eps, n_occ, n_frozen, hfx, KS=None, KT=None):
    """As cis_reference.matrices, with the exchange blocks scaled by hfx and K added (before the symmetrisation, as the reference)."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    o, v = Co.shape[1], Cv.shape[1]
    dim = o * v
    ovov = mo_tensor(E, Co, Cv, Co, Cv)
    G = ovov.reshape(dim, dim)
    X = ovov.transpose(0, 3, 2, 1).reshape(dim, dim)
    H = mo_tensor(E, Co, Co, Cv, Cv).transpose(0, 2, 1, 3).reshape(dim, dim) if hfx != 0 else np.zeros((dim, dim))
    D = np.diag((ev[None, :] - eo[:, None]).ravel())
    KS = np.zeros((dim, dim)) if KS is None else KS
    KT = np.zeros((dim, dim)) if KT is None else KT
    m = {"A_singlet": cr._sym(D + 2 * G - hfx * H + KS), "A_triplet": cr._sym(D - hfx * H + KT), "B_singlet": cr._sym(2 * G - hfx * X + KS),
         "B_triplet": cr._sym(-hfx * X + KT)}
    m["plus_singlet"], m["plus_triplet"] = m["A_singlet"] + m["B_singlet"], m["A_triplet"] + m["B_triplet"]
    m["minus"] = m["A_singlet"] - m["B_singlet"]
    return m


def solve(m, tda):
    """{"E_singlet", "E_triplet", "XpY_singlet"}: eigh of A, or the reference's 2 dim route"""
    out = {}
    for mult in ("singlet", "triplet"):
        if tda:
            e, V = cr.cis(m[f"A_{mult}"])
            out[f"E_{mult}"], out[f"XpY_{mult}"] = e, V
        else:
            e, X, Y = cr.tdhf_full(m[f"A_{mult}"], m[f"B_{mult}"])
            out[f"E_{mult}"], out[f"XpY_{mult}"] = e, X + Y
    return out


# ---- the systems of tests/golden/tddft_systems.npz (tools/make_golden_tddft.py) and their grids rebuilt -------------------------------

# tag -> (symbols, R in angstrom, basis, n_occ, functional, grid)
SYSTEMS = {
    "h2_lda_sto3g": (["H", "H"], 0.74, "STO-3G", 1, "LDA", "loose"),
    "lih_hfs_sto3g": (["LI", "H"], 1.595, "STO-3G", 2, "HFS", "loose"),
    "lih_svwn3_sto3g": (["LI", "H"], 1.595, "STO-3G", 2, "SVWN3", "loose"),
    "hf_svwn_631g": (["F", "H"], 0.917, "6-31G", 5, "SVWN", "loose"),
    "co_lda_631g": (["C", "O"], 1.128, "6-31G", 7, "LDA", "loose"),
}
EPS = np.finfo(np.float64).eps
# Two evaluations of rho(g) = sum P phi phi differ by their roundings.  The sums contribute gamma_(N^2) rho_mag (N <= 18 here: 7e-14).  An
# AO value carries the rounding of the argument of its exponentials, a r^2 eps / 2 relative, and a r^2 < 745 wherever exp(-a r^2) is
# not zero in double precision: at most 1.7e-13 per factor, two factors per term.  Together below 5e-13; the bound is 1e-12 rho_mag.
RHO_TOL = 1e-12
_REBUILT = {}


def split(z):
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def frozen_variants(g):
    return (0, 1) if int(g["n_occ"]) > 1 else (0,)


def system(tag):
    from tuna_amd import molecule as mol
    sym, R, basis, nocc, functional, grid = SYSTEMS[tag]
    atoms = mol.make_atoms(sym, mol.angstrom_to_bohr(R))
    shells = mol.build_shells(atoms, basis)
    return atoms, shells, mol.expand_cartesian_aos(shells)


def rebuilt(tag):
    """The whole grid of a system and the spherical AOs on it, built once: {"atoms", "shells", "aos", "pts" [3, G], "wts" [G],
    "phi" [G, N]} -- the grid by tuna_amd.dft.integration_grid (the one the engine is given), the AOs by xc_reference.ao_on_points."""
    if tag not in _REBUILT:
        import xc_reference as xr
        from tuna_amd import dft
        from tuna_amd.spherical import transformation_matrix
        atoms, shells, aos = system(tag)
        pts, wts, _ = dft.integration_grid(atoms, SYSTEMS[tag][5])
        pts, wts = np.asarray(pts, float).reshape(3, -1), np.asarray(wts, float).reshape(-1)
        phi, _ = xr.ao_on_points(aos, pts, transformation_matrix([s.L for s in shells]), with_grad=False)
        _REBUILT[tag] = dict(atoms=atoms, shells=shells, aos=aos, pts=pts, wts=wts, phi=phi)
    return _REBUILT[tag]


def density(phi, P):
    """(rho, the sum of the magnitudes of its N^2 terms) per grid point"""
    return np.einsum("gm,mn,gn->g", phi, P, phi, optimize=True), np.einsum("gm,mn,gn->g", np.abs(phi), np.abs(P), np.abs(phi), optimize=True)


def model_kernel(tag, g, n_frozen=0):
    """The model's K_S, K_T of a golden system on its rebuilt grid, with what their bounds need:
    {"KS", "KT", "SS", "ST" (sums of the magnitudes of the terms u T T, u by the magnitudes of ITS terms), "DS", "DT" (the first-order
    change of K when every rho(g) moves by one unit of rho_mag(g), the sum of the magnitudes of its own terms, summed in magnitude:
    sum_g |du/d ln rho| (rho_mag / rho) |T T|; RHO_TOL times this is what a density within RHO_TOL rho_mag can change), "rho", "rho_mag", "pk", "uS", "uT", "G"}."""
    r = rebuilt(tag)
    functional = SYSTEMS[tag][4]
    rho, rho_mag = density(r["phi"], g["P"])
    pk = point_kernels(rho, functional)
    uS, uT, mS, mT = weights_u(r["wts"], pk)
    T = transition_density(r["phi"], g["C"], int(g["n_occ"]), n_frozen)
    KS, SS = kernel_matrix(T, uS, mS)
    KT, ST = kernel_matrix(T, uT, mT)
    h = 1e-4                                                  # d u / d ln rho by a central difference of the closed forms
    up, dn = weights_u(r["wts"], point_kernels(pk["rho"] * (1 + h), functional)), weights_u(r["wts"], point_kernels(pk["rho"] * (1 - h), functional))
    aT = np.abs(T)
    amp = np.where(rho > FLOOR, rho_mag / pk["rho"], 0.0)     # an error of rho relative to rho_mag, as a relative error of rho (none below the floor)
    DS = (aT * (np.abs(up[0] - dn[0]) / (2 * h) * amp)) @ aT.T
    DT = (aT * (np.abs(up[1] - dn[1]) / (2 * h) * amp)) @ aT.T
    return dict(KS=KS, KT=KT, SS=SS, ST=ST, DS=DS, DT=DT, rho=pk["rho"], rho_mag=rho_mag, pk=pk, uS=uS, uT=uT, T=T, G=len(rho))


def gamma(n):
    return n * EPS / (1 - n * EPS)
