"""TEST INFRASTRUCTURE ONLY -- the restricted MP2 one-particle density in NumPy, written from the equations in chemists' notation
(include/tunafock.h: tf_mp2_density_rhf), with every MO block formed in full, the three-virtual one included.

Occupied window i, j, k = [n_frozen, n_occ), virtual a, b, c = [n_occ, N), D = e_i + e_j - e_a - e_b, G[i, a, j, b] = (ia|jb):
    tOS = -2 G / D,   tSS = (G - G^x) / D,   G^x[i, a, j, b] = (ib|ja),   w = c_os 2 G / D + c_ss 2 (G - G^x) / D
    P_ij = -1/2 c_os sum_kab tOS_kiab tOS_kjab - c_ss sum_kab tSS_kiab tSS_kjab
    P_ab = +1/2 c_os sum_ijc tOS_ijbc tOS_ijac + c_ss sum_ijc tSS_ijbc tSS_ijac
    L_ia = 2 sum_jbc w_ijbc (ab|jc) - 2 sum_jkb w_jkab (ji|kb) + 4 J[P2]_ia - 2 K[P2]_ia     (J, K of the MO-basis density P2 = P_ij + P_ab)
    (A + B)_ia,jb = delta (e_a - e_i) + 4 (ia|jb) - (ij|ab) - (ib|ja),   (A + B) z = -L,   P_ia = P_ai = z_ia / 2
and 2 on the diagonal of every occupied orbital.

Next to every value stands the sum of the magnitudes of the terms it was formed from (the same expression with |.| on every factor):
S_oo, S_vv, S_L, S_M (of A + B: |delta (e_a - e_i)| + 4 |(ia|jb)| + |(ij|ab)| + |(ib|ja)|), S_E_OS, S_E_SS, and lambda_min, norm2 of
the symmetrised A + B.  A float64 evaluation of such a sum of n terms is off by about sqrt(n) 2^-53 S, whatever cancels in it, so the
GPU tests bound |device - checker| by a multiple of S element by element (tests/test_gpu_mp2_density_shapes.py).
mp2_density_from_blocks states the same density from the four MO blocks (ia|jb), (ij|ab), (ji|kb), (ia|bc) alone.
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
    """{"E_OS", "E_SS", "P_mo", "P_ao", "L", "z", "cond"}, "P2" (P_mo without the 2 and without z) and the sums of magnitudes();
    g = mo_integrals(E, C) if the caller has it already."""
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
    out["P2"] = P2
    blocks = (G, g[o, o, v, v], g[o, o, o, v], g[o, v, v, v]) if relaxed else (G, None, None, None)
    out.update(magnitudes(eo, ev, *blocks, P2[o, o], P2[v, v], relaxed, c_os, c_ss))
    return out


def magnitudes(eo, ev, ovov, oovv, ooov, ovvv, P2oo, P2vv, relaxed, c_os, c_ss, dtype=np.float64):
    """The sums of magnitudes of the module docstring, every expression of mp2_density again with |.| on each factor:
    {"S_oo" [o, o], "S_vv" [v, v], "S_E_OS", "S_E_SS", "S_L" [o, v], "S_M" [o v, o v], "T_L" [o, v], "lambda_min", "norm2"}, the last
    five None unless relaxed.  T_L is the first-order sensitivity of L to its integrals, sum |dL_ia / dg|: integrals that are all off
    by delta move L_ia by at most delta T_L[i, a].  Blocks: ovov[i, a, j, b] = (ia|jb), oovv[i, j, a, b] = (ij|ab),
    ooov[j, i, k, b] = (ji|kb), ovvv[i, a, b, c] = (ia|bc); P2oo, P2vv the blocks of P^(2)."""
    no, nv = len(eo), len(ev)
    eo, ev = np.asarray(eo, dtype), np.asarray(ev, dtype)
    c_os, c_ss = dtype(c_os), dtype(c_ss)
    G = np.abs(np.asarray(ovov, dtype))
    Gx = G.transpose(0, 3, 2, 1)
    D = np.abs(eo[:, None, None, None] + eo[None, None, :, None] - ev[None, :, None, None] - ev[None, None, None, :])
    tos, tss = 2.0 * G / D, (G + Gx) / D
    S_oo, S_vv = np.zeros((no, no), dtype), np.zeros((nv, nv), dtype)
    for c, t, f in ((abs(c_os), tos, 0.5), (abs(c_ss), tss, 1.0)):
        S_oo += f * c * np.einsum("kaib,kajb->ij", t, t, optimize=True)
        S_vv += f * c * np.einsum("ibjc,iajc->ab", t, t, optimize=True)
    out = {"S_oo": S_oo, "S_vv": S_vv, "S_E_OS": float(np.sum(G * G / D)), "S_E_SS": float(np.sum(G * (G + Gx) / D)),
           "S_L": None, "S_M": None, "T_L": None, "lambda_min": None, "norm2": None}
    if relaxed:
        oovv, ooov, ovvv = (np.asarray(x, dtype) for x in (oovv, ooov, ovvv))
        w = abs(c_os) * 2.0 * G / D + abs(c_ss) * 2.0 * (G + Gx) / D
        Aoo, Avv, a_ooov, a_ovvv = np.abs(np.asarray(P2oo, dtype)), np.abs(np.asarray(P2vv, dtype)), np.abs(ooov), np.abs(ovvv)
        S_L = 2.0 * np.einsum("ibjc,jcab->ia", w, a_ovvv, optimize=True) + 2.0 * np.einsum("jakb,jikb->ia", w, a_ooov, optimize=True)
        S_L += 4.0 * (np.einsum("jkia,jk->ia", a_ooov, Aoo, optimize=True) + np.einsum("iabc,bc->ia", a_ovvv, Avv, optimize=True))
        S_L += 2.0 * (np.einsum("ijka,jk->ia", a_ooov, Aoo, optimize=True) + np.einsum("ibac,bc->ia", a_ovvv, Avv, optimize=True))
        S_M = (4.0 * G + np.abs(oovv).transpose(0, 2, 1, 3) + Gx).reshape(no * nv, no * nv).copy()
        S_M[np.diag_indices(no * nv)] += np.abs(ev[None, :] - eo[:, None]).ravel()
        M = _a_plus_b(eo, ev, np.asarray(ovov, dtype), oovv).astype(np.float64)
        lam = np.linalg.eigvalsh(M)
        out.update(S_L=S_L, S_M=S_M, lambda_min=float(lam[0]), norm2=float(max(abs(lam[0]), abs(lam[-1]))))
        # T_L = sum |dL_ia / dg| over every MO integral L is formed from, by the product rule on the same expression: each factor in
        # turn replaced by the magnitude of its derivative (an integral: 1; t: 2 / |D|; w: (2 |c_os| + 4 |c_ss|) / |D|)
        dt, dw = 2.0 / D, (2.0 * abs(c_os) + 4.0 * abs(c_ss)) / D
        dPoo, dPvv = np.zeros((no, no), dtype), np.zeros((nv, nv), dtype)
        for c, t, f in ((abs(c_os), tos, 0.5), (abs(c_ss), tss, 1.0)):
            dPoo += f * c * (np.einsum("kaib,kajb->ij", dt, t, optimize=True) + np.einsum("kaib,kajb->ij", t, dt, optimize=True))
            dPvv += f * c * (np.einsum("ibjc,iajc->ab", dt, t, optimize=True) + np.einsum("ibjc,iajc->ab", t, dt, optimize=True))
        T_L = 2.0 * (np.sum(w, axis=(1, 2, 3))[:, None] + np.einsum("ibjc,jcab->ia", dw, a_ovvv, optimize=True))
        T_L += 2.0 * (np.sum(w, axis=(0, 2, 3))[None, :] + np.einsum("jakb,jikb->ia", dw, a_ooov, optimize=True))
        T_L += 6.0 * (np.sum(Aoo) + np.sum(Avv))
        T_L += 4.0 * (np.einsum("jkia,jk->ia", a_ooov, dPoo, optimize=True) + np.einsum("iabc,bc->ia", a_ovvv, dPvv, optimize=True))
        T_L += 2.0 * (np.einsum("ijka,jk->ia", a_ooov, dPoo, optimize=True) + np.einsum("ibac,bc->ia", a_ovvv, dPvv, optimize=True))
        out["T_L"] = T_L
    return out


def _a_plus_b(eo, ev, ovov, oovv):
    """The symmetrised singlet A + B [o v, o v] as mp2_density forms it"""
    no, nv = len(eo), len(ev)
    M = 4.0 * ovov - oovv.transpose(0, 2, 1, 3) - ovov.transpose(0, 3, 2, 1)
    M = M.reshape(no * nv, no * nv).copy()
    M[np.diag_indices(no * nv)] += (ev[None, :] - eo[:, None]).ravel()
    return 0.5 * (M + M.T)


def mp2_density_from_blocks(eo, ev, ovov, oovv, ooov, ovvv, relaxed=False, c_os=1.0, c_ss=1.0, dtype=np.float64):
    """The outputs of mp2_density from the MO blocks of the window alone (oovv, ooov, ovvv may be None unless relaxed), no N^4 array
    formed: in the occupied-virtual block J[P2]_ia = sum_jk (ia|jk) P_jk + sum_bc (ia|bc) P_bc and K[P2]_ia = sum_jk (ij|ka) P_jk +
    sum_bc (ib|ac) P_bc.  "P_mo" is [o + v, o + v], the window and the virtuals (with the 2 on the occupied diagonal), "P2" the same
    without the 2; "P_ao" is None, there being no orbitals.  dtype = np.longdouble evaluates every contraction in extended precision
    on the same inputs (the solve stays in float64)."""
    no, nv = len(eo), len(ev)
    eo, ev = np.asarray(eo, dtype), np.asarray(ev, dtype)
    c_os, c_ss = dtype(c_os), dtype(c_ss)
    G = np.asarray(ovov, dtype)
    Gx = G.transpose(0, 3, 2, 1)
    D = eo[:, None, None, None] + eo[None, None, :, None] - ev[None, :, None, None] - ev[None, None, None, :]
    tos, tss = -2.0 * G / D, (G - Gx) / D
    Poo, Pvv = np.zeros((no, no), dtype), np.zeros((nv, nv), dtype)
    for c, t, f in ((c_os, tos, 0.5), (c_ss, tss, 1.0)):
        Poo += -f * c * np.einsum("kaib,kajb->ij", t, t, optimize=True)
        Pvv += f * c * np.einsum("ibjc,iajc->ab", t, t, optimize=True)
    out = {"E_OS": np.sum(G * G / D), "E_SS": np.sum(G * (G - Gx) / D), "L": None, "z": None, "cond": None, "D_max": float(D.max())}
    if dtype is np.float64:
        out.update(E_OS=float(out["E_OS"]), E_SS=float(out["E_SS"]))
    P2 = np.zeros((no + nv, no + nv), dtype)
    P2[:no, :no], P2[no:, no:] = Poo, Pvv
    P = P2.copy()
    P[:no, :no] += 2.0 * np.eye(no)
    if relaxed:
        oovv, ooov, ovvv = (np.asarray(x, dtype) for x in (oovv, ooov, ovvv))
        w = c_os * 2.0 * G / D + c_ss * 2.0 * (G - Gx) / D
        L = 2.0 * np.einsum("ibjc,jcab->ia", w, ovvv, optimize=True)
        L -= 2.0 * np.einsum("jakb,jikb->ia", w, ooov, optimize=True)
        J = np.einsum("jkia,jk->ia", ooov, Poo, optimize=True) + np.einsum("iabc,bc->ia", ovvv, Pvv, optimize=True)
        K = np.einsum("ijka,jk->ia", ooov, Poo, optimize=True) + np.einsum("ibac,bc->ia", ovvv, Pvv, optimize=True)
        L += 4.0 * J - 2.0 * K
        M = _a_plus_b(eo, ev, G, oovv).astype(np.float64)
        z = np.linalg.solve(M, -L.astype(np.float64).ravel()).reshape(no, nv)
        P[:no, no:] += 0.5 * z
        P[no:, :no] += 0.5 * z.T
        out.update(L=L, z=z, cond=float(np.linalg.cond(M)))
    out.update(P_mo=P, P2=P2, P_ao=None)
    out.update(magnitudes(eo, ev, ovov, oovv, ooov, ovvv, Poo, Pvv, relaxed, c_os, c_ss, dtype))
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
