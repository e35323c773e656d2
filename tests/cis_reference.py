"""Independent NumPy CIS / TDHF for the tests (no library code): the closed-shell orbital-rotation matrices from a dense spherical
(mu nu|la si) tensor and canonical RHF orbitals (occupied window [n_frozen, n_occ), virtual window [n_occ, N), compound index
(ia) = i v + a, Delta = diag(e_a - e_i)):
    singlet:  A = Delta + 2 (ia|jb) - (ij|ab),   B = 2 (ia|jb) - (ib|ja)          triplet:  A = Delta - (ij|ab),   B = -(ib|ja)
  * matrices: A and B from the dense MO blocks, each symmetrised;
  * cis: eigh of A;
  * tdhf_full: the non-symmetric 2 dim problem [[A, B], [-B, -A]], positive roots, X.X - Y.Y = 1;
  * tdhf_cholesky: A - B = L L^T, [L^T (A + B) L] Z = w^2 Z, X + Y = L Z / sqrt(w), X - Y = sqrt(w) L^-T Z, with min eig(A - B) and
    min w^2;
  * direct_products: (A +- B) b and A b from AO Coulomb / exchange contractions of T = C_o b C_v^T, with no MO block:
        sum_jb (ia|jb) b_jb = [C_o^T J(T) C_v]_ia,  sum_jb (ij|ab) b_jb = [C_o^T K(T) C_v]_ia,  sum_jb (ib|ja) b_jb = [C_o^T K(T^T) C_v]_ia,
    J(T)[mu nu] = sum (mu nu|la si) T[la si], K(T)[mu nu] = sum (mu la|nu si) T[la si];
  * transition_moments: mu_n[c] = sqrt(2) sum_ia (C_o^T D^c C_v)_ia (X + Y)^n_ia, f_n = 2/3 w_n |mu_n|^2."""
from __future__ import annotations

import numpy as np

from mp3_reference import _windows, dense_eri, mo_tensor  # noqa: F401  (dense_eri re-exported for the tests)

KINDS = ("A_singlet", "A_triplet", "plus_singlet", "plus_triplet", "minus")


def _sym(M):
    return 0.5 * (M + M.T)


def matrices(E, C, eps, n_occ, n_frozen=0):
    """{"A_singlet", "A_triplet", "B_singlet", "B_triplet", "plus_singlet", "plus_triplet", "minus"}: [dim, dim] each; plus = A + B,
    minus = A - B (the same for both multiplicities)."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    o, v = Co.shape[1], Cv.shape[1]
    dim = o * v
    ovov = mo_tensor(E, Co, Cv, Co, Cv)                      # [i a j b] = (ia|jb)
    oovv = mo_tensor(E, Co, Co, Cv, Cv)                      # [i j a b] = (ij|ab)
    G = ovov.reshape(dim, dim)
    H = oovv.transpose(0, 2, 1, 3).reshape(dim, dim)         # [(ia)][(jb)] = (ij|ab)
    X = ovov.transpose(0, 3, 2, 1).reshape(dim, dim)         # [(ia)][(jb)] = (ib|ja)
    D = np.diag((ev[None, :] - eo[:, None]).ravel())
    m = {"A_singlet": _sym(D + 2 * G - H), "A_triplet": _sym(D - H), "B_singlet": _sym(2 * G - X), "B_triplet": _sym(-X)}
    m["plus_singlet"], m["plus_triplet"] = m["A_singlet"] + m["B_singlet"], m["A_triplet"] + m["B_triplet"]
    m["minus"] = m["A_singlet"] - m["B_singlet"]
    return m


def cis(A):
    """(energies ascending, vectors [dim, dim] in columns)"""
    return np.linalg.eigh(A)


def tdhf_full(A, B):
    """(energies, X, Y) of the positive roots of [[A, B], [-B, -A]], ascending, X and Y [dim, n] in columns with X.X - Y.Y = 1."""
    n = A.shape[0]
    w, V = np.linalg.eig(np.block([[A, B], [-B, -A]]))
    w, V = w.real, V.real
    keep = w > 0
    w, V = w[keep], V[:, keep]
    order = np.argsort(w)
    w, V = w[order], V[:, order]
    X, Y = V[:n], V[n:]
    norm = np.sqrt(np.abs(np.sum(X * X, axis=0) - np.sum(Y * Y, axis=0)))
    return w, X / norm, Y / norm


def tdhf_cholesky(plus, minus):
    """{"E" ascending (NaN where w^2 <= 0), "X", "Y" [dim, dim] in columns, "min_eig_minus", "min_w2", "w2"}; X and Y are None when the
    problem has no real solution (A - B not positive definite)."""
    out = {"min_eig_minus": float(np.linalg.eigvalsh(minus)[0])}
    if out["min_eig_minus"] <= 0:
        return dict(out, E=None, X=None, Y=None, min_w2=float("nan"), w2=None)
    L = np.linalg.cholesky(minus)
    w2, Z = np.linalg.eigh(L.T @ plus @ L)
    out["min_w2"], out["w2"] = float(w2[0]), w2
    with np.errstate(invalid="ignore"):
        w = np.sqrt(w2)
    XpY = (L @ Z) / np.sqrt(w)
    XmY = np.linalg.solve(L.T, Z) * np.sqrt(w)
    return dict(out, E=w, X=0.5 * (XpY + XmY), Y=0.5 * (XpY - XmY))


def direct_products(E, C, eps, n_occ, n_frozen, b):
    """{kind: M b} for the five matrices of KINDS and trial vectors b [n, o, v], from AO Coulomb and exchange contractions alone."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    b = np.asarray(b, float)
    T = np.einsum("li,nia,sa->nls", Co, b, Cv, optimize=True)
    J = np.einsum("mnls,xls->xmn", E, T, optimize=True)
    K = np.einsum("mlns,xls->xmn", E, T, optimize=True)
    Kt = np.einsum("mlns,xsl->xmn", E, T, optimize=True)

    def mo(M):
        return np.einsum("mi,xmn,na->xia", Co, M, Cv, optimize=True)
    d = (ev[None, :] - eo[:, None])[None] * b
    return {"A_singlet": d + mo(2 * J - K), "A_triplet": d - mo(K), "plus_singlet": d + mo(4 * J - K - Kt), "plus_triplet": d - mo(K + Kt),
            "minus": d + mo(Kt - K)}


def transition_moments(D_ao, C, n_occ, n_frozen, XpY, energies):
    """(mu [n, 3], |mu| [n], f [n]) for the transition vectors X + Y [dim, n] in columns."""
    Co, Cv = np.asarray(C, float)[:, n_frozen:n_occ], np.asarray(C, float)[:, n_occ:]
    Dia = np.array([Co.T @ np.asarray(d, float) @ Cv for d in D_ao]).reshape(3, -1)
    mu = np.sqrt(2.0) * (Dia @ XpY).T
    mag = np.linalg.norm(mu, axis=1)
    return mu, mag, (2.0 / 3.0) * np.asarray(energies) * mag ** 2


def merged(E_singlet, E_triplet, mag_singlet, f_singlet):
    """The merged, sorted list of the reference (tuna_ci.py:2209-2267): (energies, labels, |mu|, f), triplets with |mu| = f = 0."""
    e = np.concatenate([E_singlet, E_triplet])
    lab = np.array(["singlet"] * len(E_singlet) + ["triplet"] * len(E_triplet))
    mu = np.concatenate([mag_singlet, np.zeros(len(E_triplet))])
    f = np.concatenate([f_singlet, np.zeros(len(E_triplet))])
    order = np.argsort(e)
    return e[order], lab[order], mu[order], f[order]


def clusters(energies, width=1e-7):
    """Index lists of consecutive states whose energies lie within `width` of their predecessor (degenerate groups)."""
    groups, cur = [], [0]
    for n in range(1, len(energies)):
        if abs(energies[n] - energies[n - 1]) < width:
            cur.append(n)
        else:
            groups.append(cur)
            cur = [n]
    groups.append(cur)
    return groups


def h2_minimal_basis(R_bohr, basis="STO-3G"):
    """(aos, E, C, eps) of the closed-shell RHF solution of H2 in a minimal basis, which symmetry fixes: sigma_g = (chi_1 + chi_2) /
    sqrt(2 + 2 S), sigma_u = (chi_1 - chi_2) / sqrt(2 - 2 S), eps = diag(C^T F C) with F = T + V + 2 J - K of P = 2 c_g c_g^T."""
    from oracle import oracle as orc
    from tuna_amd import molecule as mol
    atoms = mol.make_atoms(["H", "H"], R_bohr)
    shells = mol.build_shells(atoms, basis)
    aos = mol.expand_cartesian_aos(shells)
    S, T, V = orc.one_electron(aos, [a.origin for a in atoms], [float(a.charge) for a in atoms], [0.0, 0.0, 0.0])[:3]
    E = dense_eri(aos, shells)
    s = S[0, 1]
    C = np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt([2 + 2 * s, 2 - 2 * s])[None, :]
    P = 2.0 * np.outer(C[:, 0], C[:, 0])
    F = T + V + np.einsum("mnls,ls->mn", E, P) - 0.5 * np.einsum("mlns,ls->mn", E, P)
    return aos, E, C, np.diag(C.T @ F @ C).copy()
