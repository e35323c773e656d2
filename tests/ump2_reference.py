"""Independent NumPy UMP2 for the tests: pair energies from a dense spherical (mu nu|la si) tensor and canonical UHF orbitals, in
spatial orbitals with chemists' (ia|jb) and D = e_i + e_j - e_a - e_b (occupied windows [n_frozen_s, n_s), virtual [n_s, N)):
    E_ss = 1/2 sum (ia|jb) [(ia|jb) - (ib|ja)] / D  for s = alpha, beta;   E_ab = sum (i_a a_a|j_b b_b)^2 / D.
Not the reference's spin-orbital route (tuna_mp.py:987-1117): no (2N)^4 spin-blocked tensor, no antisymmetrised integrals."""
from __future__ import annotations

import numpy as np


def dense_eri(aos, shells):
    """The oracle's Cartesian tensor mapped to the spherical basis (the layout the library stores)."""
    from oracle import oracle as orc
    from oracle import scf_oracle as so
    from tuna_amd.spherical import transformation_matrix
    return so.eri_to_spherical(transformation_matrix([s.L for s in shells]), orc.eri(aos))


def ovov(E, Co1, Cv1, Co2, Cv2):
    """(ia|jb) = sum C1o[mu,i] C1v[nu,a] C2o[la,j] C2v[si,b] (mu nu|la si) -> [i, a, j, b]."""
    t = np.tensordot(E, Cv2, axes=(3, 0))            # mu nu la b
    t = np.tensordot(t, Co2, axes=(2, 0))            # mu nu b j
    t = np.tensordot(t, Cv1, axes=(1, 0))            # mu b j a
    t = np.tensordot(t, Co1, axes=(0, 0))            # b j a i
    return np.ascontiguousarray(t.transpose(3, 2, 1, 0))


def denominators(eo1, ev1, eo2, ev2):
    return eo1[:, None, None, None] - ev1[None, :, None, None] + eo2[None, None, :, None] - ev2[None, None, None, :]


def pair_energies(E, C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0):
    """(E_aa, E_bb, E_ab)."""
    C = {"a": np.asarray(C_alpha, float), "b": np.asarray(C_beta, float)}
    eps = {"a": np.asarray(eps_alpha, float), "b": np.asarray(eps_beta, float)}
    n = {"a": (n_frozen_alpha, n_alpha), "b": (n_frozen_beta, n_beta)}

    def occ(s):
        return C[s][:, n[s][0]:n[s][1]], eps[s][n[s][0]:n[s][1]]

    def vir(s):
        return C[s][:, n[s][1]:], eps[s][n[s][1]:]

    out = []
    for s in ("a", "b"):
        (Co, eo), (Cv, ev) = occ(s), vir(s)
        if Co.shape[1] == 0:
            out.append(0.0)
            continue
        g = ovov(E, Co, Cv, Co, Cv)
        D = denominators(eo, ev, eo, ev)
        out.append(0.5 * float(np.sum(g * (g - g.transpose(0, 3, 2, 1)) / D)))
    (Coa, eoa), (Cva, eva) = occ("a"), vir("a")
    (Cob, eob), (Cvb, evb) = occ("b"), vir("b")
    if Coa.shape[1] == 0 or Cob.shape[1] == 0:
        out.append(0.0)
    else:
        g = ovov(E, Coa, Cva, Cob, Cvb)
        out.append(float(np.sum(g * g / denominators(eoa, eva, eob, evb))))
    return tuple(out)


def frozen_split(k):
    """The reference's split of k frozen spin orbitals (tuna_mp.py:1031-1032): ceil(k/2) alpha, floor(k/2) beta."""
    return (k + 1) // 2, k // 2
