"""Independent NumPy unrestricted CIS / TDHF and orbital-Hessian spectra for the tests (no library code): the spin-blocked
orbital-rotation matrices of a UHF determinant from a dense spherical (mu nu|la si) tensor and canonical orbitals of either spin.  Per
spin s the occupied window is [n_frozen_s, n_s) and the virtual window [n_s, N); d_s = o_s v_s; the compound index holds the alpha block
first, (ia) = i v_a + a, then the beta block, d_a + j v_b + b.  With chemists' integrals,
    A[(ia s),(jb t)] = d_st d_ij d_ab (e_a - e_i) + (ia s|jb t) - d_st (ij|ab)        B[(ia s),(jb t)] = (ia s|jb t) - d_st (ib|ja)
  * matrices: A, B, A + B, A - B from the dense MO blocks (the alpha-beta rectangle of A - B comes out of the subtraction, not of a rule);
  * tdhf_cholesky / cis / tdhf_full: those of cis_reference on the spin-blocked matrices;
  * transition_moments: mu_n[c] = sum_s sum_ia (C_os^T D^c C_vs)_ia (X + Y)^n_ias -- no sqrt(2) -- and f_n = 2/3 w_n |mu_n|^2;
  * hessian_spectra_uhf / hessian_spectra_rhf: eig(A + B) and eig(A - B), whose union is the spectrum of [[A, B], [B, A]];
    full_hessian_lowest forms the matrix of order 2 dim itself, for the check of that statement."""
from __future__ import annotations

import numpy as np

import cis_reference as cr
from mp3_reference import _windows, mo_tensor


def _sym(M):
    return 0.5 * (M + M.T)


def dims(N, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0):
    """(d_alpha, d_beta)"""
    return (n_alpha - n_frozen_alpha) * (N - n_alpha), (n_beta - n_frozen_beta) * (N - n_beta)


def matrices(E, C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0):
    """{"A", "B", "plus", "minus"}: [dim, dim] each, alpha block first."""
    w = [_windows(C_alpha, eps_alpha, n_alpha, n_frozen_alpha), _windows(C_beta, eps_beta, n_beta, n_frozen_beta)]
    d = [Co.shape[1] * Cv.shape[1] for Co, Cv, _, _ in w]
    off = [0, d[0]]
    dim = d[0] + d[1]
    A, B = np.zeros((dim, dim)), np.zeros((dim, dim))
    for s, (Co, Cv, eo, ev) in enumerate(w):
        if d[s] == 0:
            continue
        sl = slice(off[s], off[s] + d[s])
        ovov = mo_tensor(E, Co, Cv, Co, Cv)                      # [i a j b] = (ia|jb)
        oovv = mo_tensor(E, Co, Co, Cv, Cv)                      # [i j a b] = (ij|ab)
        G = ovov.reshape(d[s], d[s])
        H = oovv.transpose(0, 2, 1, 3).reshape(d[s], d[s])       # [(ia)][(jb)] = (ij|ab)
        X = ovov.transpose(0, 3, 2, 1).reshape(d[s], d[s])       # [(ia)][(jb)] = (ib|ja)
        A[sl, sl] = np.diag((ev[None, :] - eo[:, None]).ravel()) + G - H
        B[sl, sl] = G - X
    if d[0] and d[1]:
        G = mo_tensor(E, w[0][0], w[0][1], w[1][0], w[1][1]).reshape(d[0], d[1])
        for M in (A, B):
            M[:d[0], d[0]:] = G
            M[d[0]:, :d[0]] = G.T
    A, B = _sym(A), _sym(B)
    return {"A": A, "B": B, "plus": A + B, "minus": A - B}


cis = cr.cis
tdhf_full = cr.tdhf_full
tdhf_cholesky = cr.tdhf_cholesky


def transition_moments(D_ao, C_alpha, C_beta, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, XpY, energies):
    """(mu [n, 3], |mu| [n], f [n]) for the transition vectors X + Y [dim, n] in columns."""
    blocks = []
    for C, n, nf in ((C_alpha, n_alpha, n_frozen_alpha), (C_beta, n_beta, n_frozen_beta)):
        Co, Cv = np.asarray(C, float)[:, nf:n], np.asarray(C, float)[:, n:]
        blocks.append(np.array([Co.T @ np.asarray(d, float) @ Cv for d in D_ao]).reshape(3, -1))
    mu = (np.concatenate(blocks, axis=1) @ XpY).T
    mag = np.linalg.norm(mu, axis=1)
    return mu, mag, (2.0 / 3.0) * np.asarray(energies) * mag ** 2


def hessian_spectra_uhf(m):
    """{"plus", "minus"} ascending, and the lowest eigenvalue of the Hessian = the smaller of their first elements"""
    s = {"plus": np.linalg.eigvalsh(m["plus"]), "minus": np.linalg.eigvalsh(m["minus"])}
    return s, float(min(s["plus"][0], s["minus"][0]))


def hessian_spectra_rhf(E, C, eps, n_occ, n_frozen=0):
    """({"plus_singlet", "plus_triplet", "minus"} ascending, lowest singlet, lowest triplet) from cis_reference.matrices"""
    m = cr.matrices(E, C, eps, n_occ, n_frozen)
    s = {k: np.linalg.eigvalsh(m[k]) for k in ("plus_singlet", "plus_triplet", "minus")}
    return s, float(min(s["plus_singlet"][0], s["minus"][0])), float(min(s["plus_triplet"][0], s["minus"][0]))


def full_hessian_lowest(A, B):
    """The lowest eigenvalue of [[A, B], [B, A]], formed as the reference forms it (order 2 dim)"""
    return float(np.linalg.eigvalsh(np.block([[A, B], [B, A]]))[0])


def energy_sorted_labels(eps_alpha, eps_beta):
    """The reference's spin-orbital labels ("3a", "2b", ...) in the combined ascending energy order (tuna_ci.py:586-603), and per spin
    the position of each of its orbitals in that order."""
    combined = np.concatenate([eps_alpha, eps_beta])
    order = np.argsort(combined)
    spins = ["a"] * len(eps_alpha) + ["b"] * len(eps_beta)
    counts, labels = {"a": 0, "b": 0}, []
    for k in order:
        counts[spins[k]] += 1
        labels.append(f"{counts[spins[k]]}{spins[k]}")
    return labels
