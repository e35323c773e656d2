"""TEST INFRASTRUCTURE ONLY -- the restricted MP2 one-particle density in NumPy, written from the equations in chemists' notation
(include/tunafock.h: tf_mp2_density_rhf), with every MO block formed in full, the three-virtual one included.

Occupied window i, j, k = [n_frozen, n_occ), virtual a, b, c = [n_occ, N), D = e_i + e_j - e_a - e_b, G[i, a, j, b] = (ia|jb):
    tOS = -2 G / D,   tSS = (G - G^x) / D,   G^x[i, a, j, b] = (ib|ja),   w = c_os 2 G / D + c_ss 2 (G - G^x) / D
    P_ij = -1/2 c_os sum_kab tOS_kiab tOS_kjab - c_ss sum_kab tSS_kiab tSS_kjab
    P_ab = +1/2 c_os sum_ijc tOS_ijbc tOS_ijac + c_ss sum_ijc tSS_ijbc tSS_ijac
    L_ia = 2 sum_jbc w_ijbc (ab|jc) - 2 sum_jkb w_jkab (ji|kb) + 4 J[P2]_ia - 2 K[P2]_ia     (J, K of the MO-basis density P2 = P_ij + P_ab)
    (A + B)_ia,jb = delta (e_a - e_i) + 4 (ia|jb) - (ij|ab) - (ib|ja),   (A + B) z = -L,   P_ia = P_ai = z_ia / 2
and 2 on the diagonal of every occupied orbital.
"""
import numpy as np

from ump2_reference import dense_eri  # noqa: F401  (re-exported: the AO tensor the tests feed in)


def mo_integrals(E, C):
    """(pq|rs) in the MO basis from the AO tensor E [N, N, N, N] (chemists' order)."""
    g = np.tensordot(E, C, axes=(3, 0))              # mu nu la s
    g = np.tensordot(g, C, axes=(2, 0))              # mu nu s r
    g = np.tensordot(g, C, axes=(1, 0))              # mu s r q
    g = np.tensordot(g, C, axes=(0, 0))              # s r q p
    return np.ascontiguousarray(g.transpose(3, 2, 1, 0))


def mp2_density(E, C, eps, n_occ, n_frozen=0, relaxed=False, c_os=1.0, c_ss=1.0, g=None):
    """{"E_OS", "E_SS", "P_mo", "P_ao", "L", "z", "cond"}; g = mo_integrals(E, C) if the caller has it already."""
    N = len(eps)
    g = mo_integrals(E, C) if g is None else g
    o, v = slice(n_frozen, n_occ), slice(n_occ, N)
    no, nv = n_occ - n_frozen, N - n_occ
    eo, ev = eps[o], eps[v]
    G = g[o, v, o, v]                                                    # [i, a, j, b] = (ia|jb)
    Gx = G.transpose(0, 3, 2, 1)                                         # [i, a, j, b] = (ib|ja)
    D = eo[:, None, None, None] + eo[None, None, :, None] - ev[None, :, None, None] - ev[None, None, None, :]
    tos, tss = -2.0 * G / D, (G - Gx) / D
    P2 = np.zeros((N, N))
    for c, t, f in ((c_os, tos, 0.5), (c_ss, tss, 1.0)):
        P2[o, o] += -f * c * np.einsum("kaib,kajb->ij", t, t, optimize=True)
        P2[v, v] += f * c * np.einsum("ibjc,iajc->ab", t, t, optimize=True)
    out = {"E_OS": float(np.sum(G * G / D)), "E_SS": float(np.sum(G * (G - Gx) / D)), "L": None, "z": None, "cond": None}
    P = P2.copy()
    P[:n_occ, :n_occ] += 2.0 * np.eye(n_occ)
    if relaxed:
        if n_frozen != 0:
            raise ValueError("the relaxed density needs n_frozen = 0")
        w = c_os * 2.0 * G / D + c_ss * 2.0 * (G - Gx) / D               # [i, a, j, b] = w_ijab
        L = 2.0 * np.einsum("ibjc,abjc->ia", w, g[v, v, o, v], optimize=True)
        L -= 2.0 * np.einsum("jakb,jikb->ia", w, g[o, o, o, v], optimize=True)
        J = np.einsum("pqrs,rs->pq", g, P2, optimize=True)
        K = np.einsum("prqs,rs->pq", g, P2, optimize=True)
        L += (4.0 * J - 2.0 * K)[o, v]
        M = 4.0 * G - g[o, o, v, v].transpose(0, 2, 1, 3) - Gx            # [i, a, j, b]
        M = M.reshape(no * nv, no * nv).copy()
        M[np.diag_indices(no * nv)] += (ev[None, :] - eo[:, None]).ravel()
        M = 0.5 * (M + M.T)
        z = np.linalg.solve(M, -L.ravel()).reshape(no, nv)
        P[o, v] += 0.5 * z
        P[v, o] += 0.5 * z.T
        out.update(L=L, z=z, cond=float(np.linalg.cond(M)))
    out["P_mo"] = P
    out["P_ao"] = C @ P @ C.T
    return out


def stencil(E, h):
    """dE/dF at F = 0 from E(F) at F = -2h, -h, +h, +2h: the four-point central difference, error O(h^4)."""
    return (8.0 * (E(h) - E(-h)) - (E(2.0 * h) - E(-2.0 * h))) / (12.0 * h)


def field_system(atoms, shells, aos):
    """One-electron matrices (spherical), the z dipole matrix about the centre of mass, the AO tensor and what a cycle needs."""
    from oracle import oracle as orc
    from oracle import scf_oracle as so
    from tuna_amd import guess as guess_mod
    from tuna_amd import molecule as mol
    from tuna_amd.spherical import transformation_matrix
    U = transformation_matrix([s.L for s in shells])
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    com = guess_mod.centre_of_mass(atoms) if len(atoms) == 2 else 0.0
    S, T, V, D, _ = orc.one_electron(aos, xyz, chg, [0.0, 0.0, com])
    S, T, V, Dz = (so.to_spherical(U, M) for M in (S, T, V, D[2]))
    X = so.orthogonaliser(S)[0]
    ranges = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    return dict(S=S, T=T, V=V, Dz=Dz, X=X, E=so.eri_to_spherical(U, orc.eri(aos)), V_NN=mol.nuclear_repulsion(atoms), ranges=ranges)


def cpu_field_energy(sysd, n_occ, F):
    """E_RHF + E_MP2 with F D_z added to the core Hamiltonian: oracle/scf_oracle.py's cycle at EXTREME thresholds from the core guess."""
    from oracle import scf_oracle as so
    P0, E0 = so.core_guess(sysd["T"], sysd["V"], sysd["X"], n_occ)
    r = so.run_rhf(sysd["S"], sysd["T"], sysd["V"], sysd["E"], sysd["X"], P0, E0, n_occ, sysd["V_NN"], sysd["ranges"], conv="extreme",
                   Fext=F * sysd["Dz"])
    d = mp2_density(sysd["E"], r["C"], r["epsilons"], n_occ)
    return r["energy"] + d["E_OS"] + d["E_SS"]


def natural_orbitals(P, X):
    """(occupations descending, orbitals) of X^-1 P X^-T."""
    Xi = np.linalg.inv(X)
    M = Xi @ P @ Xi.T
    w, V = np.linalg.eigh(0.5 * (M + M.T))
    return w[::-1], (X @ V)[:, ::-1]
